// dict.hip — chunk dicts (PackOption.ChunkDictPath, builder.go:122-124) as
// reference-counted HBM objects, and their C ABI (include/nydus_gpu.h): storage
// and handles, create, extend, retire, distill, fold, export and probe.  Loading one from
// a bootstrap file, and the engine's open cache, are dict_load.hip.  A Pack pins
// the dict it was opened with, so packs against different dicts can be open on
// one engine at once.
//
// Layout in HBM per dict of m entries (table order): 64-B records (digest,
// usize, blob, index, global id, uoff), hash slots u64[next_pow2(2m+16)] (open
// addressing, dedup.hip).  The compressed placement a layer's DICT records copy
// (offset, size, flags) stays on the host: only the blob writer reads it.
// Records, table and placement rows belong to a reference-counted DictStorage;
// a handle is immutable, and ngpu_dict_extend ("dict extend" below) puts a new
// handle on the same storage when there is room, else on a larger one; so do
// ngpu_dict_fold and ngpu_dict_extend_device ("dict fold"), whose new records
// are written by a kernel from tables that already lie in HBM.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "blob.hpp"
#include "dict_fold_plan.hpp"
#include "dict_grow_plan.hpp"
#include "dict_retire_plan.hpp"
#include "engine_internal.hpp"
#include "host_window.hpp"

using namespace ngpu;

namespace ngpu {

void node_dict_free(ngpu_dict *d);  // node.hip

void dict_ref(ngpu_dict *d) {
  if (d) d->refs.fetch_add(1, std::memory_order_relaxed);
}

// The last handle on a storage frees it: handles of one storage share its
// records and table, so nothing is freed while any of them can still be probed.
void storage_unref(DictStorage *st) {
  if (!st || st->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  DeviceGuard g(st->device);
  // hipFree waits for the device, so no queued probe still reads the table
  if (st->rec) (void)hipFree(st->rec);
  if (st->table) (void)hipFree(st->table);
  free(st->place);
  delete st;
}

void dict_unref(ngpu_dict *d) {
  if (!d || d->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  if (!d->req.empty() || !d->parts.empty()) node_dict_free(d);
  storage_unref(d->st);
  delete d;
}

int dict_check(ngpu_engine *e, const ngpu_dict *d) {
  if (!d) return 0;
  bool here = d->device == e->device;
  for (const ngpu_dict *p : d->parts) here = here || p->device == e->device;  // node dicts
  if (!here)
    return fail(e, NGPU_EINVAL, "chunk dict lives on device %d, engine on %d", d->device, e->device);
  if (d->digester != e->cfg.digester)
    return fail(e, NGPU_EINVAL, "inconsistent digester: chunk dict %s vs engine %s",
                d->digester ? "sha256" : "blake3", e->cfg.digester ? "sha256" : "blake3");
  if (d->chunk_size != e->cfg.chunk_size)
    return fail(e, NGPU_EINVAL, "inconsistent chunk size: chunk dict 0x%x vs engine 0x%x",
                d->chunk_size, e->cfg.chunk_size);
  return 0;
}

ngpu_dict *default_dict(ngpu_engine *e) {  // e->mu held
  dict_ref(e->dict);
  return e->dict;
}

// A storage of rec_cap record slots and table_cap hash slots (place: with host
// placement rows), none of them reserved yet.  The rows are malloc'ed, not
// zeroed: the pages past the last row written are never touched.
int storage_alloc(ngpu_engine *e, uint64_t rec_cap, uint64_t table_cap, bool place,
                  DictStorage **out) {
  DictStorage *st = new DictStorage();
  st->device = e->device;
  st->rec_cap = rec_cap;
  st->table_cap = table_cap;
  const uint64_t bytes[2] = {rec_cap * sizeof(DictRec), table_cap * 8};
  void *p[2] = {};
  for (int i = 0; i < 2; ++i) {
    if (hipMalloc(&p[i], bytes[i] ? bytes[i] : 64) != hipSuccess) {
      (void)hipGetLastError();
      if (p[0]) (void)hipFree(p[0]);
      delete st;
      return fail(e, NGPU_ENOMEM, "chunk dict: %llu entries do not fit in HBM",
                  (unsigned long long)rec_cap);
    }
  }
  st->rec = (DictRec *)p[0];
  st->table = (uint64_t *)p[1];
  if (place && rec_cap && !(st->place = (DictPlace *)malloc(rec_cap * sizeof(DictPlace)))) {
    storage_unref(st);
    return fail(e, NGPU_ENOMEM, "chunk dict: no host memory for %llu placement rows",
                (unsigned long long)rec_cap);
  }
  *out = st;
  return 0;
}

// Point d at entries [0, m) of the storage it holds.
void dict_bind(ngpu_dict *d, uint64_t m, uint32_t n_blobs) {
  DictDevice &v = d->dev;
  v.rec = d->st->rec;
  v.table = d->st->table;
  v.mask = d->st->table_cap - 1;
  v.m = m;
  v.n_blobs = n_blobs;
}

// Allocate the records and hash table of an m-entry dict: a storage of its
// own, exactly its size and all of it reserved.
int dict_alloc(ngpu_engine *e, ngpu_dict *d, uint64_t m, uint32_t n_blobs, bool place) {
  if (int rc = storage_alloc(e, m, next_pow2(2 * m + 16), place, &d->st)) return rc;
  d->st->used = m;
  d->has_place = place && m;
  dict_bind(d, m, n_blobs);
  return 0;
}

ngpu_dict *dict_new(ngpu_engine *e) {
  ngpu_dict *d = new ngpu_dict();
  d->device = e->device;
  d->digester = e->cfg.digester;
  d->chunk_size = e->cfg.chunk_size;
  return d;
}

ngpu_dict *dict_derive(const ngpu_dict *base) {
  ngpu_dict *d = new ngpu_dict();
  d->device = base->device;
  d->digester = base->digester;
  d->chunk_size = base->chunk_size;
  d->replicated = base->replicated;
  d->routed = base->routed;
  return d;
}

// A dict build runs on a stream of its own, outside the engine lock: a load
// of a 200M-entry bootstrap takes seconds, and under e->mu (round 3) it stalled
// every Pack of the engine for that long, while its stream syncs on the
// engine's own stream waited for their work too.
BuildStream::BuildStream(int device) {
  DeviceGuard g(device);
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    s = nullptr;
  }
}
BuildStream::~BuildStream() {
  if (s) (void)hipStreamDestroy(s);
}

void place_rows_from_records(const uint8_t *recs, uint64_t k, DictPlace *dst) {
  for (uint64_t i = 0; i < k; ++i) {
    const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
    dst[i] = DictPlace{r->compressed_offset, r->compressed_size, r->flags};
  }
}

int blob_count_verdict(ngpu_engine *e, uint64_t seen, uint32_t n_blobs, uint32_t *nb) {
  if (n_blobs) {
    if (seen > n_blobs)
      return fail(e, NGPU_EFORMAT, "chunk dict record points at blob %u of %u", (uint32_t)(seen - 1),
                  n_blobs);
    seen = n_blobs;
  }
  if (seen > (1u << 20))
    return fail(e, NGPU_EINVAL, "chunk dict blob index %u too large", (uint32_t)(seen - 1));
  *nb = (uint32_t)seen;
  return 0;
}

int records_blob_count(ngpu_engine *e, const uint8_t *recs, uint64_t k, uint32_t n_blobs,
                       uint32_t *nb) {
  uint64_t seen = 0;  // (64 bits: index 0xFFFFFFFF + 1 does not wrap to "no blob")
  for (uint64_t i = 0; i < k; ++i) {
    const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
    seen = std::max<uint64_t>(seen, (uint64_t)r->blob_index + 1);
  }
  return blob_count_verdict(e, seen, n_blobs, nb);
}

void dict_merge_blob_table(ngpu_dict *d, const ngpu_dict *base, bool with_table,
                           const uint8_t *blobs, uint32_t n_blobs) {
  if (!with_table) return;
  d->blob_table = base->blob_table;
  if (blobs && n_blobs) d->blob_table.insert(d->blob_table.end(), blobs, blobs + 256ull * n_blobs);
}

int dict_plain_base_check(ngpu_engine *e, const ngpu_dict *base, const char *what,
                          const char *node_hint) {
  if (!base->parts.empty()) return fail(e, NGPU_EINVAL, "%s: %s", what, node_hint);
  if (base->device != e->device)
    return fail(e, NGPU_EINVAL, "chunk dict lives on device %d, engine on %d", base->device,
                e->device);
  return dict_check(e, base);
}

int grow_kept(ngpu_engine *e, uint8_t **ptr, uint64_t *cap, uint64_t bytes, const char *msg) {
  if (bytes <= *cap) return 0;
  // (nothing of an earlier fold still runs: each is complete when it returns)
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  const uint64_t want = std::max<uint64_t>(bytes + bytes / 2, 1u << 16);
  if (hipMalloc((void **)ptr, want) != hipSuccess) {
    (void)hipGetLastError();
    *ptr = nullptr;
    return fail(e, NGPU_ENOMEM, "%s", msg);
  }
  *cap = want;
  return 0;
}

int storage_alloc_place_only(ngpu_engine *e, uint64_t cap, DictStorage **out) {
  DictStorage *st = new DictStorage();
  st->device = e->device;
  st->rec_cap = cap;
  st->table_cap = ~0ull;
  if (cap && !(st->place = (DictPlace *)malloc(cap * sizeof(DictPlace)))) {
    delete st;
    return fail(e, NGPU_ENOMEM, "chunk dict: no host memory for %llu placement rows",
                (unsigned long long)cap);
  }
  *out = st;
  return 0;
}

namespace {

// NGPU_DICT_TRACE=1: one stderr line per extend, fold, retire or distill with its device
// time between HIP events (tools/dict_*_bench.py read them); off: no event is made.
struct DictTrace {
  hipEvent_t ev[5] = {};
  bool on = false;
  static bool enabled() {
    static const bool t = [] {
      const char *v = getenv("NGPU_DICT_TRACE");
      return v && v[0] == '1';
    }();
    return t;
  }
  explicit DictTrace(int n, bool want = true) {
    if (!want || !enabled()) return;
    on = true;
    for (int i = 0; i < n; ++i)
      if (hipEventCreate(&ev[i]) != hipSuccess) ev[i] = nullptr, on = false;
  }
  ~DictTrace() {
    for (hipEvent_t x : ev)
      if (x) (void)hipEventDestroy(x);
  }
  void record(int i, hipStream_t s) {
    if (on) (void)hipEventRecord(ev[i], s);
  }
  // microseconds from event i to event j, both complete; < 0: not timed
  double us(int i, int j) const {
    float ms = 0;
    return on && hipEventElapsedTime(&ms, ev[i], ev[j]) == hipSuccess ? ms * 1000.0 : -1.0;
  }
};

// dict_upload_unpack's staging buffers; hipFree waits for the device, so they outlive the caller's sync.
struct DictStaging {
  uint8_t *tmp = nullptr;
  uint32_t *tmp_gid = nullptr;
  int reserve(ngpu_engine *e, uint64_t k, bool with_gids) {
    const uint64_t batch = std::min<uint64_t>(k, 1u << 20);
    if (!k || tmp) return 0;
    if (hipMalloc((void **)&tmp, batch * 80) != hipSuccess ||
        (with_gids && hipMalloc((void **)&tmp_gid, batch * 4) != hipSuccess)) {
      (void)hipGetLastError();
      return fail(e, NGPU_ENOMEM, "chunk dict: staging allocation failed");
    }
    return 0;
  }
  ~DictStaging() {
    if (tmp_gid) (void)hipFree(tmp_gid);
    if (tmp) (void)hipFree(tmp);
  }
};

// k host 80-B records into dst_rec[0, k) on s, in batches of <= 1M through stg: gid =
// gids[i] (null: gid0 + i), blob0 added to every blob index.  Synced between batches, not
// after the last (the caller's sync serves).  first(): after the first upload, before its launch.
template <class First>
int dict_upload_unpack(ngpu_engine *e, DictStaging &stg, const uint8_t *recs, const uint32_t *gids,
                       uint64_t k, uint32_t gid0, uint32_t blob0, DictRec *dst_rec, hipStream_t s,
                       First first) {
  if (int rc = stg.reserve(e, k, gids != nullptr)) return rc;
  const uint64_t batch = std::min<uint64_t>(k, 1u << 20);
  for (uint64_t a = 0; a < k; a += batch) {
    const uint64_t c = std::min(batch, k - a);
    if (hipMemcpyAsync(stg.tmp, recs + 80 * a, c * 80, hipMemcpyHostToDevice, s) != hipSuccess ||
        (gids && hipMemcpyAsync(stg.tmp_gid, gids + a, c * 4, hipMemcpyHostToDevice, s) != hipSuccess))
      return fail(e, NGPU_EHIP, "chunk dict: upload failed");
    if (a == 0) first();
    launch_dict_unpack(stg.tmp, c, gids ? stg.tmp_gid : nullptr, gid0 + (uint32_t)a, dst_rec + a, s,
                       blob0);
    if (a + c < k && hipStreamSynchronize(s) != hipSuccess)
      return fail(e, NGPU_EHIP, "chunk dict: unpack failed");
  }
  return 0;
}

}  // namespace

// Build the hash table over the uploaded digests (first table entry wins).
int dict_build(ngpu_engine *e, ngpu_dict *d, hipStream_t s) {
  launch_dict_build(d->dev.rec, d->dev.m, const_cast<uint64_t *>(d->dev.table), d->dev.mask + 1, s);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipStreamSynchronize(s));
  return 0;
}

// From 80-B RAFS v6 chunk records in host memory (no engine lock needed: the
// upload and build run on their own stream); gids: the records' global entry
// ids (node shards), null = their positions.
int dict_from_records(ngpu_engine *e, const uint8_t *recs, uint64_t m, const uint8_t *blobs,
                      uint32_t n_blobs, ngpu_dict **out, const uint32_t *gids) {
  DeviceGuard dg(e->device);
  BuildStream bs(e->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  if (m >= 0xFFFFFFFFull) return fail(e, NGPU_EINVAL, "chunk dict too large (%llu entries)",
                                      (unsigned long long)m);
  uint32_t nb = 0;
  if (int rc = records_blob_count(e, recs, m, n_blobs, &nb)) return rc;
  ngpu_dict *d = dict_new(e);
  int rc = dict_alloc(e, d, m, nb, true);
  if (rc) {
    dict_unref(d);
    return rc;
  }
  place_rows_from_records(recs, m, d->st->place);
  if (blobs && n_blobs) d->blob_table.assign(blobs, blobs + 256ull * n_blobs);
  DictStaging stg;
  rc = dict_upload_unpack(e, stg, recs, gids, m, 0, 0, const_cast<DictRec *>(d->dev.rec), bs.s, [] {});
  if (!rc) rc = dict_build(e, d, bs.s);
  if (rc) {
    dict_unref(d);
    return rc;
  }
  *out = d;
  return 0;
}

// SoA arrays (host or device memory, `kind`) -> dict (no engine lock; own
// stream, like dict_from_records).
int dict_from_arrays(ngpu_engine *e, const uint8_t *dg, const uint32_t *us, const uint32_t *bl,
                     const uint32_t *ix, const uint64_t *uo, uint64_t m, uint32_t n_blobs,
                     hipMemcpyKind kind, ngpu_dict **out, const uint32_t *gid = nullptr) {
  DeviceGuard dgd(e->device);
  BuildStream bs(e->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  if (m >= 0xFFFFFFFFull) return fail(e, NGPU_EINVAL, "chunk dict too large (%llu entries)",
                                      (unsigned long long)m);
  if (n_blobs > (1u << 20)) return fail(e, NGPU_EINVAL, "chunk dict blob index %u too large",
                                        n_blobs - 1);
  ngpu_dict *d = dict_new(e);
  int rc = dict_alloc(e, d, m, n_blobs, false);
  if (rc) {
    dict_unref(d);
    return rc;
  }
  DictRec *rec = const_cast<DictRec *>(d->dev.rec);
  if (m && kind == hipMemcpyHostToDevice) {  // pack on the host, one upload
    std::vector<DictRec> h(m);
    for (uint64_t i = 0; i < m; ++i) {
      DictRec &r = h[i];
      memset(&r, 0, sizeof r);
      memcpy(r.digest, dg + 32 * i, 32);
      r.usize = us[i];
      r.blob = bl[i];
      r.index = ix ? ix[i] : 0;
      r.gid = gid ? gid[i] : (uint32_t)i;
      r.uoff = uo ? uo[i] : 0;
    }
    if (hipMemcpyAsync(rec, h.data(), m * sizeof(DictRec), kind, bs.s) != hipSuccess ||
        hipStreamSynchronize(bs.s) != hipSuccess)
      rc = fail(e, NGPU_EHIP, "chunk dict: upload failed");
  } else if (m) {
    launch_dict_pack(dg, us, bl, ix, uo, gid, m, 0, 0, rec, bs.s);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "chunk dict: pack failed");
  }
  if (!rc) rc = dict_build(e, d, bs.s);
  if (rc) {
    dict_unref(d);
    return rc;
  }
  *out = d;
  return 0;
}

// ---- dict extend ---------------------------------------------------------------
// A handle never changes; ngpu_dict_extend returns a new one that answers as a
// dict created from the concatenation would.  When the base is the newest
// handle on its storage and the storage has room (dict_grow_plan.hpp) the k
// records are appended in place: the unpack kernel writes rec[m, m + k), then a
// second launch inserts ids m .. m + k - 1 into the live table.  Older handles
// (and kernels probing them on other streams meanwhile) do not see any of it:
// new entries take only slots that were empty, never displace an entry and
// never win an atomicMin against a smaller id, so an old handle's chain still
// ends where it ended or walks over new slots, which dict_find skips unread
// because their id is >= the handle's m.  Otherwise the result goes onto a new
// storage half as large again: base's records copied device to device, the new
// ones unpacked behind them, the table built over all of them.

int dict_extend_check(ngpu_engine *e, const ngpu_dict *base, const uint8_t *recs, uint64_t k,
                      const uint8_t *blobs, uint32_t n_blobs, uint32_t *nb_out, bool *with_table) {
  const uint64_t m = base->dev.m;
  if (m >= kDictMaxEntries || k >= kDictMaxEntries - m)
    return fail(e, NGPU_EINVAL, "chunk dict too large (%llu entries)", (unsigned long long)(m + k));
  uint32_t nb = 0;
  if (int rc = records_blob_count(e, recs, k, n_blobs, &nb)) return rc;
  return dict_extend_check_blobs(e, base, k, nb, blobs && n_blobs, n_blobs, nb_out, with_table);
}

// The half of dict_extend_check that needs no records (a fold counts its blobs
// on the device): nb more blobs against the 2^20 limit, and the blob table rule
// (dict_fold_plan.hpp): kept only when both sides have one; a base of 0 blobs
// goes with either, and so does a call that adds nothing.
int dict_extend_check_blobs(ngpu_engine *e, const ngpu_dict *base, uint64_t k, uint32_t nb,
                            bool call_has, uint32_t n_blobs, uint32_t *nb_out, bool *with_table) {
  const uint64_t m = base->dev.m;
  if (m >= kDictMaxEntries || k >= kDictMaxEntries - m)
    return fail(e, NGPU_EINVAL, "chunk dict too large (%llu entries)", (unsigned long long)(m + k));
  if (nb > (1u << 20) || base->dev.n_blobs + nb > (1u << 20))
    return fail(e, NGPU_EINVAL, "chunk dict blob index %u too large", base->dev.n_blobs + nb - 1);
  const DictTableRule r =
      dict_table_rule(base->dev.n_blobs, !base->blob_table.empty(), call_has, k, n_blobs);
  if (r < 0)
    return fail(e, NGPU_EINVAL,
                r == kTableBaseOnly
                    ? "dict extend: the base has a blob table, the new records come without one"
                    : "dict extend: the base has no blob table, the new records come with one");
  *with_table = r == kTableKept;
  *nb_out = base->dev.n_blobs + nb;
  return 0;
}

int dict_extend_records(ngpu_engine *e, ngpu_dict *base, const uint8_t *recs, uint64_t k,
                        uint32_t blob0, uint32_t nb, const uint32_t *gids, bool place,
                        ngpu_dict **out) {
  DictRowSource src;
  src.recs = recs;
  src.gids = gids;
  src.blob0 = blob0;
  return dict_extend_rows(e, base, src, k, nb, place, out);
}

int dict_extend_rows(ngpu_engine *e, ngpu_dict *base, const DictRowSource &src, uint64_t k,
                     uint32_t nb, bool place, ngpu_dict **out) {
  DeviceGuard dg(e->device);
  DictStorage *st = base->st;
  const uint64_t m = base->dev.m;
  const uint8_t *recs = src.recs;
  const uint32_t *gids = src.gids;
  const bool staged = !src.write;  // host records: upload + unpack
  const bool want_place = place && (base->has_place || m == 0);
  DictGrowPlan plan;
  bool share = k == 0;  // nothing to write: another handle on the same entries
  if (k) {
    std::lock_guard<std::mutex> g(st->mu);
    plan = dict_grow_plan(m, st->used, st->rec_cap, st->table_cap, k);
    if (!plan.ok)
      return fail(e, NGPU_EINVAL, "chunk dict too large (%llu entries)", (unsigned long long)(m + k));
    if (plan.share && want_place && !st->place)  // (an empty handle on a storage without rows)
      plan = dict_grow_plan(m, m + 1, st->rec_cap, st->table_cap, k);
    share = plan.share;
    // the id range [m, m + k) is this call's from here on; if the call fails it
    // stays dead: no handle reaches it and nobody appends to this storage again
    if (share) st->used = m + k;
  }
  DictStorage *dst = st;
  if (!share) {
    if (int rc = storage_alloc(e, plan.rec_cap, plan.table_cap, want_place, &dst)) return rc;
    dst->used = m + k;
  } else {
    st->refs.fetch_add(1, std::memory_order_relaxed);
  }
  int rc = 0;
  if (k) {
    // a device source brings the stream its inputs are ordered on
    std::unique_ptr<BuildStream> own(src.stream ? nullptr : new BuildStream(e->device));
    const hipStream_t bs = src.stream ? src.stream : own->s;
    DictStaging stg;
    if (!bs)
      rc = fail(e, NGPU_EHIP, "chunk dict: no build stream");
    else if (staged)
      rc = stg.reserve(e, k, gids != nullptr);
    // the trace line's device time: an in-place append from before its first
    // launch (after the records' upload) to the end of the inserts, a copy from
    // before the device-to-device copy to the end of the table build
    DictTrace tr(2, !rc);
    if (!share) tr.record(0, bs);
    if (!rc && !share && m &&
        hipMemcpyAsync(dst->rec, st->rec, m * sizeof(DictRec), hipMemcpyDeviceToDevice, bs) !=
            hipSuccess)
      rc = fail(e, NGPU_EHIP, "chunk dict: copy of the base's records failed");
    if (!rc && want_place) {
      if (!share && base->has_place) memcpy(dst->place, st->place, m * sizeof(DictPlace));
      if (staged)
        place_rows_from_records(recs, k, dst->place + m);
      else if (src.rows)
        memcpy(dst->place + m, src.rows, k * sizeof(DictPlace));
    }
    // launch 1: rec[m, m + k) from the 80-B records (per batch of <= 1M; one
    // batch: the sync after the inserts serves), or (device source) by its own kernel
    if (staged && !rc) {
      rc = dict_upload_unpack(e, stg, recs, gids, k, (uint32_t)m, src.blob0, dst->rec + m, bs, [&] {
        if (share) tr.record(0, bs);
      });
    } else if (!rc) {
      if (share) tr.record(0, bs);
      src.write(dst->rec + m, m, bs);
      if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "chunk dict: record write failed");
    }
    // launch 2, after every record is written: the new ids into the live table
    // (share), or the whole table of the new storage (fork)
    if (!rc) {
      if (share)
        launch_dict_insert_range(dst->rec, m, m + k, dst->table, dst->table_cap, bs);
      else
        launch_dict_build(dst->rec, m + k, dst->table, dst->table_cap, bs);
      if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "chunk dict: table insert failed");
    }
    tr.record(1, bs);
    if (bs && hipStreamSynchronize(bs) != hipSuccess && !rc)
      rc = fail(e, NGPU_EHIP, "chunk dict: extend failed");
    const double us = rc ? -1.0 : tr.us(0, 1);
    if (us >= 0 && staged)
      fprintf(stderr, "ngpu dict_extend %s m=%llu k=%llu device_us=%.1f\n", share ? "share" : "fork",
              (unsigned long long)m, (unsigned long long)k, us);
    else if (us >= 0)  // the fold's keep + scan ran before the counts came back
      fprintf(stderr, "ngpu %s %s m=%llu k=%llu n=%llu device_us=%.1f keep_scan_us=%.1f\n", src.name,
              share ? "share" : "fork", (unsigned long long)m, (unsigned long long)k,
              (unsigned long long)src.n, us + src.pre_us, src.pre_us);
  }
  if (rc) {
    storage_unref(dst);
    return rc;
  }
  ngpu_dict *d = dict_derive(base);
  d->st = dst;
  d->has_place = want_place && m + k;
  d->shares_base = share;
  dict_bind(d, m + k, nb);
  *out = d;
  return 0;
}

// recs: 80-B records, or (null) rows: their placement rows.
static int place_extend(ngpu_engine *e, ngpu_dict *base, const uint8_t *recs, const DictPlace *rows,
                        uint64_t k, ngpu_dict *out) {
  const uint64_t m = base ? base->dev.m : 0;
  DictStorage *st = base ? base->st : nullptr;
  const bool base_rows = base && base->has_place && st && st->place;
  if (m && !base_rows) return 0;  // base keeps no rows: neither does the result
  bool share = false;
  DictGrowPlan plan;
  if (st) {
    std::lock_guard<std::mutex> g(st->mu);
    plan = dict_grow_plan(m, st->used, st->rec_cap, ~0ull, k);
    share = plan.ok && plan.share && (st->place || k == 0);
    if (share && k) st->used = m + k;
  }
  if (share) {
    st->refs.fetch_add(1, std::memory_order_relaxed);
  } else {
    // creation (no base): exactly k rows; a fork: half as many again
    const uint64_t cap = st ? dict_grow_plan(m, m + 1, 0, 0, k).rec_cap : k;
    if (int rc = storage_alloc_place_only(e, cap, &st)) return rc;
    st->used = m + k;
    if (base_rows) memcpy(st->place, base->st->place, m * sizeof(DictPlace));
  }
  if (recs)
    place_rows_from_records(recs, k, st->place + m);
  else if (k)
    memcpy(st->place + m, rows, k * sizeof(DictPlace));
  out->st = st;
  out->has_place = m + k != 0;
  return 0;
}

int dict_place_extend(ngpu_engine *e, ngpu_dict *base, const uint8_t *recs, uint64_t k,
                      ngpu_dict *out) {
  return place_extend(e, base, recs, nullptr, k, out);
}

int dict_place_extend(ngpu_engine *e, ngpu_dict *base, const DictPlace *rows, uint64_t k,
                      ngpu_dict *out) {
  return place_extend(e, base, nullptr, rows, k, out);
}

// ---- dict retire ---------------------------------------------------------------
// The reverse of an extend: a new handle of base's records without those of the
// listed blobs, as a dict created from the surviving rows would be.  Nothing of
// base's storage is written (a probe of base on another stream reads what it
// always read), so the result always sits on a storage of its own, with the
// room a fork leaves (dict_retire_plan.hpp): launches 1-2 (dict_retire.hip) give
// every record a keep bit and every 64 records the number of survivors before
// them, the host reads the total and allocates, launch 3 moves the survivors,
// launch 4 is the table build every dict gets.  The placement rows are compacted
// on the host by the same keep words and prefixes, on the host pipelines' thread
// pool (host_window.hpp), while launches 3-4 run: one thread's walk over 200M
// bits, with the page faults of 3 GB of fresh rows, took 0.7 s against 19 ms on
// the device (DESIGN.md §3 "Dict retire").

void dict_retire_place(const DictKeep &keep, uint64_t m, const DictPlace *src, DictPlace *dst,
                       uint64_t s) {
  const uint64_t nw = (m + 63) / 64;
  const uint64_t pieces = (nw + kRetireHostPiece - 1) / kRetireHostPiece;
  const uint64_t *words = keep.words.data();
  const uint32_t *prefix = keep.prefix.data();
  run_indexed(host_threads(0), pieces, [=](uint64_t q) {
    dict_retire_compact_rows(words, prefix, q * kRetireHostPiece,
                             std::min(nw, (q + 1) * kRetireHostPiece), m, src, dst, s);
  });
}

std::vector<uint8_t> dict_retire_blob_table(const std::vector<uint8_t> &table,
                                            const std::vector<uint32_t> &remap) {
  std::vector<uint8_t> t;
  if (table.empty()) return t;
  for (size_t b = 0; b < remap.size() && 256 * (b + 1) <= table.size(); ++b)
    if (remap[b] != kRetiredBlob) t.insert(t.end(), table.begin() + 256 * b, table.begin() + 256 * (b + 1));
  return t;
}

// What a retire and a distill share once the keep words, their prefixes, the
// survivor total s and the blob remap lie in HBM (and hk holds the host copy of
// the words and prefixes when rows are to be moved): the storage of the result,
// launches 3-4 between events ev and ev + 1 of tr, the placement rows on the host
// pool meanwhile, and the sync.  *dst: the storage, s of its slots used.
static int dict_compact_tail(ngpu_engine *e, const char *what, const ngpu_dict *base, hipStream_t bs,
                             const uint64_t *d_words, const uint32_t *d_cnt, const uint32_t *d_remap,
                             uint64_t s, const DictPlace *place, const DictKeep &hk, DictTrace &tr,
                             int ev, DictStorage **dst_out) {
  const uint64_t m = base->dev.m;
  DictStorage *dst = nullptr;
  int rc = 0;
  if (s > m) rc = fail(e, NGPU_EHIP, "%s: %llu survivors of %llu records", what,
                       (unsigned long long)s, (unsigned long long)m);
  if (!rc)
    rc = storage_alloc(e, dict_retire_rec_cap(s), dict_retire_table_cap(s), place && s, &dst);
  if (!rc) {
    dst->used = s;
    tr.record(ev, bs);
    launch_dict_compact(base->st ? base->st->rec : nullptr, m, d_words, d_cnt, d_remap,
                        base->dev.n_blobs, dst->rec, s, bs);
    launch_dict_build(dst->rec, s, dst->table, dst->table_cap, bs);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "%s: compaction failed", what);
    tr.record(ev + 1, bs);
  }
  // the placement rows, while the device moves the records
  if (!rc && place && s) dict_retire_place(hk, m, place, dst->place, s);
  if (hipStreamSynchronize(bs) != hipSuccess && !rc)
    rc = fail(e, NGPU_EHIP, "%s: compaction failed", what);
  if (rc) {
    storage_unref(dst);
    return rc;
  }
  *dst_out = dst;
  return 0;
}

// The handle of a compaction's result: s entries and nb blobs on dst.
static ngpu_dict *dict_compact_handle(const ngpu_dict *base, DictStorage *dst, uint64_t s, uint32_t nb,
                                      bool place) {
  ngpu_dict *d = dict_derive(base);
  d->st = dst;
  d->has_place = place && s;
  dict_bind(d, s, nb);
  return d;
}

int dict_retire_records(ngpu_engine *e, const ngpu_dict *base, const std::vector<uint32_t> &bitmap,
                        const std::vector<uint32_t> &remap, uint32_t nb, const DictPlace *place,
                        DictKeep *keep, ngpu_dict **out) {
  DeviceGuard dg(e->device);
  const uint64_t m = base->dev.m;
  const uint32_t nb0 = base->dev.n_blobs;
  const uint64_t nw = (m + 63) / 64, nt = dict_retire_scan_tiles(m);
  BuildStream bs(e->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  const RetireScratch lay = retire_scratch_layout(m, bitmap.size(), remap.size());
  uint8_t *scr = nullptr;
  if (hipMalloc((void **)&scr, lay.bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, NGPU_ENOMEM, "dict retire: scratch allocation failed");
  }
  uint64_t *d_words = (uint64_t *)(scr + lay.words), *d_sums = (uint64_t *)(scr + lay.sums);
  uint32_t *d_cnt = (uint32_t *)(scr + lay.cnt), *d_bits = (uint32_t *)(scr + lay.bits),
           *d_remap = (uint32_t *)(scr + lay.remap);
  // the trace line's device time: launches 1-2 plus launches 3-4 (the allocation
  // between them is host time)
  DictTrace tr(4);
  int rc = 0;
  DictStorage *dst = nullptr;
  DictKeep own_keep;
  DictKeep &hk = keep ? *keep : own_keep;
  uint64_t s = 0;
  if (hipMemcpyAsync(d_bits, bitmap.data(), 4 * bitmap.size(), hipMemcpyHostToDevice, bs.s) != hipSuccess ||
      (!remap.empty() && hipMemcpyAsync(d_remap, remap.data(), 4 * remap.size(),
                                        hipMemcpyHostToDevice, bs.s) != hipSuccess))
    rc = fail(e, NGPU_EHIP, "dict retire: upload failed");
  if (!rc) {
    tr.record(0, bs.s);
    launch_dict_keep_scan(base->st ? base->st->rec : nullptr, m, d_bits, nb0, d_words, d_cnt, d_sums,
                          bs.s);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "dict retire: keep scan failed");
    tr.record(1, bs.s);
  }
  if (!rc && (place || keep) && nw) {
    hk.words.resize(nw);
    hk.prefix.resize(nw);
    if (hipMemcpyAsync(hk.words.data(), d_words, 8 * nw, hipMemcpyDeviceToHost, bs.s) != hipSuccess ||
        hipMemcpyAsync(hk.prefix.data(), d_cnt, 4 * nw, hipMemcpyDeviceToHost, bs.s) != hipSuccess)
      rc = fail(e, NGPU_EHIP, "dict retire: keep words did not come back");
  }
  if (!rc && (hipMemcpyAsync(&s, d_sums + nt, 8, hipMemcpyDeviceToHost, bs.s) != hipSuccess ||
              hipStreamSynchronize(bs.s) != hipSuccess))
    rc = fail(e, NGPU_EHIP, "dict retire: keep scan failed");
  if (!rc) {
    rc = dict_compact_tail(e, "dict retire", base, bs.s, d_words, d_cnt, d_remap, s, place, hk, tr, 2, &dst);
  } else if (hipStreamSynchronize(bs.s) != hipSuccess) {
    (void)hipGetLastError();  // (nothing of the stream still reads the scratch)
  }
  const double a = rc ? -1.0 : tr.us(0, 1), b = rc ? -1.0 : tr.us(2, 3);
  if (a >= 0 && b >= 0)
    fprintf(stderr, "ngpu dict_retire m=%llu s=%llu device_us=%.1f keep_scan_us=%.1f compact_build_us=%.1f\n",
            (unsigned long long)m, (unsigned long long)s, a + b, a, b);
  (void)hipFree(scr);
  if (rc) return rc;
  *out = dict_compact_handle(base, dst, s, nb, place != nullptr);
  return 0;
}

// ---- dict distill --------------------------------------------------------------
// A retire whose keep bits come from the rows themselves: a row stays when it is
// the first of its digest and at least min_refs rows hold that digest
// (dict_distill.hip counts them through the table the base already has).  One
// mid-way copy brings the survivor total, the counters of the info and the
// blob-live bitmap back; the host turns the bitmap into the blob remap
// (dict_distill_plan.hpp), uploads it, and the rest is retire's tail.  table: the
// blob rows MERGE_BLOB_IDS compares (the node handle's for a replica).

int dict_distill_records(ngpu_engine *e, const ngpu_dict *base, const std::vector<uint8_t> &table,
                         uint32_t min_refs, uint32_t flags, const DictPlace *place, DictKeep *keep,
                         bool want_out, DictDistilled *res, ngpu_dict **out) {
  DeviceGuard dg(e->device);
  const uint64_t m = base->dev.m;
  const uint32_t nb0 = base->dev.n_blobs;
  const uint64_t nw = (m + 63) / 64;
  if (nb0 > kDictMaxBlobs) return fail(e, NGPU_EINVAL, "dict distill: a dict of %u blobs", nb0);
  BuildStream bs(e->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  const DistillScratch lay = distill_scratch_layout(m, nb0);
  uint8_t *scr = nullptr;
  if (hipMalloc((void **)&scr, lay.bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, NGPU_ENOMEM, "dict distill: scratch allocation failed");
  }
  uint64_t *d_words = (uint64_t *)(scr + lay.words), *d_sums = (uint64_t *)(scr + lay.sums),
           *d_stats = (uint64_t *)(scr + lay.stats);
  uint32_t *d_cnt = (uint32_t *)(scr + lay.cnt), *d_live = (uint32_t *)(scr + lay.live),
           *d_remap = (uint32_t *)(scr + lay.remap), *d_refs = (uint32_t *)(scr + lay.refs);
  const DictRec *rec = base->st ? base->st->rec : nullptr;
  // the trace line's device time: launch 1, launches 2-5, and the tail's two
  DictTrace tr(5);
  int rc = 0;
  DictStorage *dst = nullptr;
  DictKeep own_keep;
  DictKeep &hk = keep ? *keep : own_keep;
  std::vector<uint8_t> back(lay.back_bytes);
  if (hipMemsetAsync(scr + lay.back, 0, lay.back_bytes, bs.s) != hipSuccess ||
      (m && hipMemsetAsync(d_refs, 0, 4 * m, bs.s) != hipSuccess))
    rc = fail(e, NGPU_EHIP, "dict distill: clearing the counters failed");
  if (!rc) {
    tr.record(0, bs.s);
    launch_dict_ref_count(rec, m, base->st ? base->st->table : nullptr,
                          base->st ? base->st->table_cap : 0, d_refs, bs.s);
    tr.record(1, bs.s);
    launch_distill_keep_scan(rec, m, d_refs, min_refs, nb0, d_words, d_cnt, d_sums, d_live, d_stats,
                             bs.s);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "dict distill: counting failed");
    tr.record(2, bs.s);
  }
  if (!rc && want_out && (place || keep) && nw) {
    hk.words.resize(nw);
    hk.prefix.resize(nw);
    if (hipMemcpyAsync(hk.words.data(), d_words, 8 * nw, hipMemcpyDeviceToHost, bs.s) != hipSuccess ||
        hipMemcpyAsync(hk.prefix.data(), d_cnt, 4 * nw, hipMemcpyDeviceToHost, bs.s) != hipSuccess)
      rc = fail(e, NGPU_EHIP, "dict distill: keep words did not come back");
  }
  // the survivor total, the counters and the live blobs: the call's one mid-way copy
  if (!rc && (hipMemcpyAsync(back.data(), scr + lay.back, lay.back_bytes, hipMemcpyDeviceToHost, bs.s) !=
                  hipSuccess ||
              hipStreamSynchronize(bs.s) != hipSuccess))
    rc = fail(e, NGPU_EHIP, "dict distill: counting failed");
  uint64_t s = 0;
  uint64_t stats[kDistillStatWords] = {};
  if (!rc) {
    memcpy(&s, back.data(), 8);
    memcpy(stats, back.data() + (lay.stats - lay.back), sizeof stats);
    if (!distill_stats_sane(stats, m, s))
      rc = fail(e, NGPU_EHIP, "dict distill: %llu survivors, %llu digests of %llu records",
                (unsigned long long)s, (unsigned long long)stats[kDistillDistinct], (unsigned long long)m);
  }
  if (!rc) {
    res->plan = distill_blob_plan(nb0, reinterpret_cast<const uint32_t *>(back.data() + (lay.live - lay.back)),
                                  flags, table.size() >= 256ull * nb0 && nb0 ? table.data() : nullptr);
    distill_info_fill(&res->info, m, stats, nb0, res->plan.n_kept);
    res->s = s;
  }
  if (!rc && want_out) {
    if (nb0 && hipMemcpyAsync(d_remap, res->plan.remap.data(), 4ull * nb0, hipMemcpyHostToDevice, bs.s) !=
                   hipSuccess)
      rc = fail(e, NGPU_EHIP, "dict distill: upload failed");
    if (!rc)
      rc = dict_compact_tail(e, "dict distill", base, bs.s, d_words, d_cnt, d_remap, s, place, hk, tr, 3,
                             &dst);
  }
  if (rc && hipStreamSynchronize(bs.s) != hipSuccess)
    (void)hipGetLastError();  // (nothing of the stream still reads the scratch)
  const double a = rc ? -1.0 : tr.us(0, 1), b = rc ? -1.0 : tr.us(1, 2),
               c = rc || !want_out ? 0.0 : tr.us(3, 4);
  if (a >= 0 && b >= 0 && c >= 0)
    fprintf(stderr,
            "ngpu dict_distill m=%llu s=%llu device_us=%.1f count_us=%.1f keep_scan_us=%.1f "
            "compact_build_us=%.1f\n",
            (unsigned long long)m, (unsigned long long)s, a + b + c, a, b, c);
  (void)hipFree(scr);
  if (rc) return rc;
  if (want_out) *out = dict_compact_handle(base, dst, s, res->plan.n_kept, place != nullptr);
  return 0;
}

int dict_distill_args(uint32_t flags) {
  const uint32_t both = NGPU_DICT_DISTILL_KEEP_BLOBS | NGPU_DICT_DISTILL_MERGE_BLOB_IDS;
  return (flags & ~both) || (flags & both) == both ? NGPU_EINVAL : 0;
}

void dict_export_row(const DictRec &r, const DictPlace *row, uint8_t *dst) {
  RafsV6ChunkInfo x;
  memset(&x, 0, sizeof x);
  memcpy(x.block_id, r.digest, 32);
  x.blob_index = r.blob;
  x.uncompressed_size = r.usize;
  x.uncompressed_offset = r.uoff;
  x.index = r.index;
  if (row) {
    x.compressed_offset = row->compressed_offset;
    x.compressed_size = row->compressed_size;
    x.flags = row->flags;
  } else {  // as ngpu_dict_load documents: stored uncompressed at offset 0
    x.compressed_size = r.usize;
  }
  memcpy(dst, &x, 80);
}

// The handle's own rows back as 80-B RAFS v6 chunk-info records: the HBM rows of
// p (a plain dict or a replica) in pieces of 1M, the placement rows of `rows`.
static int dict_export_records(ngpu_engine *e, const ngpu_dict *p, const DictPlace *rows,
                               uint8_t *records) {
  const uint64_t m = p->dev.m;
  if (!m) return 0;
  DeviceGuard dg(p->device);
  BuildStream bs(p->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  const uint64_t batch = std::min<uint64_t>(m, 1u << 20);
  std::vector<DictRec> h(batch);
  for (uint64_t a = 0; a < m; a += batch) {
    const uint64_t c = std::min(batch, m - a);
    if (hipMemcpyAsync(h.data(), p->st->rec + a, c * sizeof(DictRec), hipMemcpyDeviceToHost, bs.s) !=
            hipSuccess ||
        hipStreamSynchronize(bs.s) != hipSuccess)
      return fail(e, NGPU_EHIP, "dict export: copy of the records failed");
    for (uint64_t i = 0; i < c; ++i) dict_export_row(h[i], rows ? rows + a + i : nullptr, records + 80 * (a + i));
  }
  return 0;
}

}  // namespace ngpu

extern "C" {

int ngpu_dict_create(ngpu_engine *e, const void *records, uint64_t n, const void *blob_table,
                     uint32_t n_blobs, ngpu_dict **out) {
  if (!e || !out || (n && !records) || (n_blobs && !blob_table)) return NGPU_EINVAL;
  *out = nullptr;
  return guarded([&] {
    return dict_from_records(e, (const uint8_t *)records, n, (const uint8_t *)blob_table, n_blobs,
                             out, nullptr);
  });
}

}  // extern "C"

int ngpu::dict_extend(ngpu_engine *e, ngpu_dict *base, const uint8_t *recs, uint64_t n,
                      const uint8_t *blobs, uint32_t n_blobs, ngpu_dict **out) {
  if (int rc = dict_plain_base_check(e, base, "dict extend",
                                     "a node dict is extended with ngpu_node_dict_extend"))
    return rc;
  uint32_t nb = 0;
  bool with_table = false;
  if (int rc = dict_extend_check(e, base, recs, n, blobs, n_blobs, &nb, &with_table)) return rc;
  ngpu_dict *d = nullptr;
  if (int rc = dict_extend_records(e, base, recs, n, base->dev.n_blobs, nb, nullptr, true, &d))
    return rc;
  dict_merge_blob_table(d, base, with_table, blobs, n_blobs);
  *out = d;
  return 0;
}

extern "C" {

int ngpu_dict_extend(ngpu_engine *e, ngpu_dict *base, const void *records, uint64_t n,
                     const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !e || !out || (n && !records) || (n_blobs && !blob_table))
    return NGPU_EINVAL;
  return guarded([&] {
    return dict_extend(e, base, (const uint8_t *)records, n, (const uint8_t *)blob_table, n_blobs,
                       out);
  });
}

// ---- dict fold -----------------------------------------------------------------
// An extend whose records never leave HBM (dict_fold.hip): the source of
// dict_extend_rows is a kernel that writes rec[m, m + k) from the call's result
// table (ngpu_dict_fold) or from SoA arrays (ngpu_dict_extend_device), so the
// share / fork decision, the storage and the handle are extend's own.  A fold
// learns k and its blob count from the device: launches 1-3 run first, one 64-B
// copy brings the counters back (the call's only mid-way sync), everything is
// checked on the host, and only then is `used` reserved and a storage written.
// Both calls run on the engine's fold stream with its kept scratch (fold_mu):
// no device allocation or free on the in-place path.

static_assert(sizeof(ngpu_dict_place) == sizeof(DictPlace) &&
                  offsetof(ngpu_dict_place, compressed_size) == offsetof(DictPlace, compressed_size) &&
                  offsetof(ngpu_dict_place, flags) == offsetof(DictPlace, flags),
              "ngpu_dict_place is a DictPlace");

}  // extern "C"

// e->fold_mu held: the fold stream, and at least `bytes` of scratch.
int ngpu::fold_lane(ngpu_engine *e, uint64_t bytes) {
  if (!e->fold_stream &&
      hipStreamCreateWithFlags(&e->fold_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    e->fold_stream = nullptr;
    return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  }
  return grow_kept(e, &e->fold_scr, &e->fold_scr_cap, bytes, "dict fold: scratch allocation failed");
}

int ngpu::fold_fail(ngpu_engine *e, const char *prefix, const FoldVerdict &v, uint64_t n, uint64_t L) {
  switch (v.why) {
    case FoldVerdict::ok: return 0;
    case FoldVerdict::bad_layer:
      return fail(e, NGPU_EINVAL,
                  "%slayer_first is not 0 = first[0] <= ... <= first[%llu] = %llu at layer %llu", prefix,
                  (unsigned long long)L, (unsigned long long)n, (unsigned long long)v.which);
    case FoldVerdict::bad_kind:
      return fail(e, NGPU_EINVAL,
                  "%schunk %llu is no dedup result (its kind is none of NEW / INTRA / DICT; "
                  "%llu such chunks)",
                  prefix, (unsigned long long)v.which, (unsigned long long)v.count);
    case FoldVerdict::bad_len:
      return fail(e, NGPU_EINVAL,
                  "%sNEW chunk %llu has length 0 or more than chunk size 0x%x (%llu such chunks)", prefix,
                  (unsigned long long)v.which, e->cfg.chunk_size, (unsigned long long)v.count);
    case FoldVerdict::insane: break;
  }
  return fail(e, NGPU_EHIP, "%s%llu NEW chunks in %llu layers of %llu chunks", prefix,
              (unsigned long long)v.k, (unsigned long long)v.b, (unsigned long long)n);
}

int ngpu::fold_place_fail(ngpu_engine *e, const char *prefix, DictFoldPlace pr, uint64_t n_placements,
                          uint64_t k, bool rows_ok, uint32_t n_blobs, uint64_t b) {
  if (pr == kPlaceCount)
    return fail(e, NGPU_EINVAL, "%s%llu placements for %llu NEW chunks", prefix,
                (unsigned long long)n_placements, (unsigned long long)k);
  if (pr == kPlaceMissing)
    return fail(e, NGPU_EINVAL, "%sthe base keeps compressed placements, the call gives none", prefix);
  if (pr == kPlaceUnwanted)
    return fail(e, NGPU_EINVAL, "%sthe base keeps no compressed placements, the call gives some",
                prefix);
  if (!rows_ok)
    return fail(e, NGPU_EINVAL, "%sa blob table of %u rows for %llu layers with a NEW chunk", prefix,
                n_blobs, (unsigned long long)b);
  return 0;
}

static int dict_extend_device(ngpu_engine *e, ngpu_dict *base, const uint8_t *dg, const uint32_t *us,
                              const uint32_t *bl, const uint32_t *ix, const uint64_t *uo, uint64_t n,
                              uint32_t n_blobs, ngpu_dict **out) {
  if (int rc = dict_plain_base_check(e, base, "dict extend_device", "node dicts are not supported"))
    return rc;
  ngpu_dict *d = nullptr;
  if (n == 0) {  // a handle equal to base
    if (int rc = dict_extend_rows(e, base, DictRowSource{}, 0, base->dev.n_blobs, base->has_place, &d))
      return rc;
    d->blob_table = base->blob_table;
    *out = d;
    return 0;
  }
  uint32_t nb = 0;
  bool with_table = false;
  if (int rc = dict_extend_check_blobs(e, base, n, n_blobs, false, n_blobs, &nb, &with_table))
    return rc;
  if (base->has_place)
    return fail(e, NGPU_EINVAL,
                "dict extend_device: the base keeps compressed placements, device arrays carry none");
  std::lock_guard<std::mutex> lane(e->fold_mu);
  DeviceGuard dgd(e->device);
  if (int rc = fold_lane(e, 0)) return rc;
  const uint32_t blob0 = base->dev.n_blobs;
  auto write = [&](DictRec *dst, uint64_t m, hipStream_t s) {
    launch_dict_pack(dg, us, bl, ix, uo, nullptr, n, blob0, (uint32_t)m, dst, s);
  };
  DictRowSource src;
  src.write = std::ref(write);  // (a reference: no allocation for the captures)
  src.stream = e->fold_stream;
  src.name = "dict_extend_device";
  src.n = n;
  if (int rc = dict_extend_rows(e, base, src, n, nb, false, &d)) return rc;
  *out = d;
  return 0;
}

static int dict_fold(ngpu_engine *e, ngpu_dict *base, const ngpu_result *d_res,
                     const ngpu_chunk *d_chunks, uint64_t n, const uint64_t *d_lfirst, uint64_t L,
                     const ngpu_dict_place *placements, uint64_t n_placements, const uint8_t *blobs,
                     uint32_t n_blobs, ngpu_dict **out) {
  if (int rc = dict_plain_base_check(e, base, "dict fold", "node dicts are not supported")) return rc;
  if (n >= kDictMaxEntries || L >= kDictMaxEntries)
    return fail(e, NGPU_EINVAL, "dict fold: %llu chunks in %llu layers in one call",
                (unsigned long long)n, (unsigned long long)L);
  if (L <= 1) d_lfirst = nullptr, L = 1;  // one layer of n chunks
  std::lock_guard<std::mutex> lane(e->fold_mu);
  DeviceGuard dg(e->device);
  const FoldScratch lay = fold_scratch_layout(n, L, 8 * kFoldCtrWords);
  if (int rc = fold_lane(e, lay.bytes)) return rc;
  const hipStream_t s = e->fold_stream;
  uint8_t *scr = e->fold_scr;
  uint64_t *d_words = (uint64_t *)(scr + lay.words), *d_sums = (uint64_t *)(scr + lay.sums),
           *d_ctr = (uint64_t *)(scr + lay.ctr);
  uint32_t *d_cnt = (uint32_t *)(scr + lay.cnt), *d_rank = (uint32_t *)(scr + lay.rank);
  uint64_t ctr[kFoldCtrWords] = {};
  int rc = 0;
  double pre_us = 0;
  {
    DictTrace tr(2);  // launches 1-3
    if (hipMemsetAsync(d_ctr, 0, 8 * kFoldCtrWords, s) != hipSuccess)
      rc = fail(e, NGPU_EHIP, "dict fold: keep scan failed");
    if (!rc) {
      tr.record(0, s);
      launch_fold_keep_scan(d_res, d_chunks, n, e->cfg.chunk_size, d_lfirst, L, d_words, d_cnt, d_sums,
                            d_rank, d_ctr, s);
      if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "dict fold: keep scan failed");
      tr.record(1, s);
    }
    // k, b and the refusals in one small copy: the call's only mid-way sync
    if (!rc && (hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess))
      rc = fail(e, NGPU_EHIP, "dict fold: keep scan failed");
    if (!rc) pre_us = std::max(0.0, tr.us(0, 1));
  }
  if (rc) return rc;
  // every check below comes before `used` is reserved or a storage byte is written
  const FoldVerdict v = fold_counts_verdict(ctr, n, L);
  if (int r = fold_fail(e, "dict fold: ", v, n, L)) return r;
  const uint64_t k = v.k, b = v.b;
  const DictFoldPlace pr =
      dict_fold_place_rule(base->dev.m, base->has_place, placements != nullptr, n_placements, k);
  if (int r = fold_place_fail(e, "dict fold: ", pr, n_placements, k, !blobs || n_blobs == b, n_blobs, b))
    return r;
  uint32_t nb = 0;
  bool with_table = false;
  if (int r = dict_extend_check_blobs(e, base, k, (uint32_t)b, blobs && n_blobs, n_blobs, &nb, &with_table))
    return r;
  ngpu_dict *d = nullptr;
  if (k == 0) {  // a handle equal to base
    rc = dict_extend_rows(e, base, DictRowSource{}, 0, base->dev.n_blobs, base->has_place, &d);
  } else {
    const uint32_t blob0 = base->dev.n_blobs;
    auto write = [&](DictRec *dst, uint64_t m, hipStream_t ws) {
      launch_fold_scatter(d_res, d_chunks, n, d_words, d_cnt, d_lfirst, L, d_rank, blob0, (uint32_t)m,
                          dst, k, ws);
    };
    DictRowSource src;
    src.write = std::ref(write);  // (a reference: no allocation for the captures)
    src.rows = reinterpret_cast<const DictPlace *>(placements);
    src.stream = s;
    src.name = "dict_fold";
    src.pre_us = (float)pre_us;
    src.n = n;
    rc = dict_extend_rows(e, base, src, k, nb, pr == kPlaceKept, &d);
  }
  if (rc) return rc;
  dict_merge_blob_table(d, base, with_table, blobs, n_blobs);
  *out = d;
  return 0;
}

extern "C" {

int ngpu_dict_extend_device(ngpu_engine *e, ngpu_dict *base, const uint8_t *d_digests,
                            const uint32_t *d_usize, const uint32_t *d_blob_index,
                            const uint32_t *d_chunk_index, const uint64_t *d_uoff, uint64_t n,
                            uint32_t n_blobs, uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !e || !out || (n && (!d_digests || !d_usize || !d_blob_index)) ||
      ((uintptr_t)d_digests & 15))
    return NGPU_EINVAL;
  return guarded([&] {
    return dict_extend_device(e, base, d_digests, d_usize, d_blob_index, d_chunk_index, d_uoff, n,
                              n_blobs, out);
  });
}

int ngpu_dict_fold(ngpu_engine *e, ngpu_dict *base, const ngpu_result *d_results,
                   const ngpu_chunk *d_chunks, uint64_t n, const uint64_t *d_layer_first,
                   uint64_t n_layers, const ngpu_dict_place *placements, uint64_t n_placements,
                   const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !e || !out || (n && (!d_results || !d_chunks)) ||
      ((uintptr_t)d_results & 15) || ((uintptr_t)d_chunks & 7) || ((uintptr_t)d_layer_first & 7) ||
      (n_placements && !placements) || (n_blobs && !blob_table))
    return NGPU_EINVAL;
  return guarded([&] {
    return dict_fold(e, base, d_results, d_chunks, n, d_layer_first, n_layers, placements,
                     n_placements, (const uint8_t *)blob_table, n_blobs, out);
  });
}

int ngpu_dict_retire(ngpu_engine *e, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                     uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !e || !out || (n && !blobs)) return NGPU_EINVAL;
  return guarded([&]() -> int {
    if (int rc = dict_plain_base_check(e, base, "dict retire",
                                       "a node dict is retired with ngpu_node_dict_retire"))
      return rc;
    const DictRetirePlan plan = dict_retire_plan(base->dev.n_blobs, blobs, n);
    if (!plan.ok)
      return fail(e, NGPU_EINVAL, "dict retire: blob %u of a dict of %u blobs", plan.bad,
                  base->dev.n_blobs);
    ngpu_dict *d = nullptr;
    if (int rc = dict_retire_records(e, base, plan.bitmap, plan.remap, plan.n_kept, base->place(),
                                     nullptr, &d))
      return rc;
    d->blob_table = dict_retire_blob_table(base->blob_table, plan.remap);
    *out = d;
    return 0;
  });
}

int ngpu_dict_distill(ngpu_engine *e, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                      ngpu_dict **out, ngpu_dict_distill_info *info) {
  if (out) *out = nullptr;
  if (info) memset(info, 0, sizeof *info);
  if (!base || !e || dict_distill_args(flags)) return NGPU_EINVAL;
  return guarded([&]() -> int {
    if (int rc = dict_plain_base_check(e, base, "dict distill",
                                       "a node dict is distilled with ngpu_node_dict_distill"))
      return rc;
    if ((flags & NGPU_DICT_DISTILL_MERGE_BLOB_IDS) && base->dev.m && base->blob_table.empty())
      return fail(e, NGPU_EINVAL, "dict distill: blob ids are merged by the blob table, the dict has none");
    DictDistilled res;
    ngpu_dict *d = nullptr;
    if (int rc = dict_distill_records(e, base, base->blob_table, min_refs, flags, base->place(), nullptr,
                                      out != nullptr, &res, &d))
      return rc;
    if (d) d->blob_table = dict_retire_blob_table(base->blob_table, res.plan.rows);
    if (out) *out = d;
    if (info) *info = res.info;
    return 0;
  });
}

int ngpu_dict_export(ngpu_engine *e, const ngpu_dict *d, void *records, uint64_t cap,
                     uint64_t *n_records, void *blob_table, uint32_t blob_cap, uint32_t *n_blobs) {
  if (n_records) *n_records = d ? d->dev.m : 0;
  if (n_blobs) *n_blobs = d ? d->dev.n_blobs : 0;
  if (!e || !d || !n_records || !n_blobs) return NGPU_EINVAL;
  return guarded([&]() -> int {
    if (!d->parts.empty() && !d->replicated)
      return fail(e, NGPU_EUNSUPP,
                  "dict export: a partitioned node dict's rows lie on its parts (not supported yet)");
    const ngpu_dict *p = d->parts.empty() ? d : d->parts[0];
    const uint64_t m = d->dev.m;
    if (!records && !cap) return 0;  // a count
    if (cap < m || (m && !records))
      return fail(e, NGPU_EINVAL, "dict export: room for %llu of %llu records",
                  (unsigned long long)cap, (unsigned long long)m);
    const bool table = blob_table && !d->blob_table.empty();
    if (table && 256ull * blob_cap < d->blob_table.size())
      return fail(e, NGPU_EINVAL, "dict export: room for %u of %llu blob records", blob_cap,
                  (unsigned long long)(d->blob_table.size() / 256));
    if (p->dev.m != m) return fail(e, NGPU_EINVAL, "dict export: replica of %llu entries, dict of %llu",
                                   (unsigned long long)p->dev.m, (unsigned long long)m);
    if (int rc = dict_export_records(e, p, d->place(), (uint8_t *)records)) return rc;
    if (table) memcpy(blob_table, d->blob_table.data(), d->blob_table.size());
    return 0;
  });
}

int ngpu_dict_info_get(const ngpu_dict *d, ngpu_dict_info *out) {
  if (!d || !out) return NGPU_EINVAL;
  memset(out, 0, sizeof *out);
  const ngpu_dict *p = d->parts.empty() ? d : d->parts[0];
  out->entries = d->dev.m;
  out->blobs = d->dev.n_blobs;
  if (p->st) {
    out->record_capacity = p->st->rec_cap;
    out->table_capacity = p->st->table_cap;
  }
  out->shares_base_storage = p->shares_base;
  out->has_blob_table = !d->blob_table.empty();
  return 0;
}

int ngpu_dict_create_device(ngpu_engine *e, const uint8_t *d_digests, const uint32_t *d_usize,
                            const uint32_t *d_blob_index, const uint32_t *d_chunk_index,
                            const uint64_t *d_uoff, uint64_t n, uint32_t n_blobs,
                            ngpu_dict **out) {
  return ngpu_dict_create_device_gid(e, d_digests, d_usize, d_blob_index, d_chunk_index, d_uoff,
                                     nullptr, n, n_blobs, out);
}

int ngpu_dict_create_device_gid(ngpu_engine *e, const uint8_t *d_digests, const uint32_t *d_usize,
                                const uint32_t *d_blob_index, const uint32_t *d_chunk_index,
                                const uint64_t *d_uoff, const uint32_t *d_gid, uint64_t n,
                                uint32_t n_blobs, ngpu_dict **out) {
  if (!e || !out || (n && (!d_digests || !d_usize || !d_blob_index))) return NGPU_EINVAL;
  *out = nullptr;
  if (n_blobs == 0 || n_blobs > (1u << 20)) return fail(e, NGPU_EINVAL, "bad n_blobs %u", n_blobs);
  return guarded([&] {
    return dict_from_arrays(e, d_digests, d_usize, d_blob_index, d_chunk_index, d_uoff, n, n_blobs,
                            hipMemcpyDeviceToDevice, out, d_gid);
  });
}

void ngpu_dict_retain(ngpu_dict *d) { dict_ref(d); }
void ngpu_dict_release(ngpu_dict *d) { dict_unref(d); }
uint64_t ngpu_dict_entries(const ngpu_dict *d) { return d ? d->dev.m : 0; }

int ngpu_set_dict(ngpu_engine *e, ngpu_dict *d) {
  if (!e) return NGPU_EINVAL;
  ngpu_dict *old;
  {
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = dict_check(e, d)) return rc;
    dict_ref(d);
    old = e->dict;
    e->dict = d;
  }
  dict_unref(old);  // outside the lock; packs that captured it keep their own reference
  return 0;
}

int ngpu_dict_load(ngpu_engine *e, const uint8_t *digests, const uint32_t *usize,
                   const uint32_t *blob_index, const uint32_t *chunk_index, uint64_t n) {
  if (!e || (n && (!digests || !usize || !blob_index))) return NGPU_EINVAL;
  ngpu_dict *d = nullptr;
  {
    uint32_t nb = 0;
    for (uint64_t i = 0; i < n; ++i) nb = std::max(nb, blob_index[i] + 1);
    if (int rc = guarded([&] {
          return dict_from_arrays(e, digests, usize, blob_index, chunk_index, nullptr, n, nb,
                                  hipMemcpyHostToDevice, &d);
        }))
      return rc;
  }
  const int rc = ngpu_set_dict(e, n ? d : nullptr);
  dict_unref(d);
  return rc;
}

int ngpu_dict_load_device(ngpu_engine *e, const uint8_t *d_digests, const uint32_t *d_usize,
                          const uint32_t *d_blob_index, const uint32_t *d_chunk_index,
                          uint64_t n, uint32_t n_blobs) {
  ngpu_dict *d = nullptr;
  int rc = ngpu_dict_create_device(e, d_digests, d_usize, d_blob_index, d_chunk_index, nullptr, n,
                                   n_blobs, &d);
  if (rc) return rc;
  rc = ngpu_set_dict(e, n ? d : nullptr);
  dict_unref(d);
  return rc;
}

int ngpu_dict_load_bootstrap(ngpu_engine *e, const char *path) {
  ngpu_dict *d = nullptr;
  int rc = ngpu_dict_open(e, path, &d);
  if (rc) return rc;
  rc = ngpu_set_dict(e, d);
  dict_unref(d);
  return rc;
}

int ngpu_dict_clear(ngpu_engine *e) { return ngpu_set_dict(e, nullptr); }

uint64_t ngpu_dict_size(const ngpu_engine *e) {
  if (!e) return 0;
  std::lock_guard<std::mutex> g(const_cast<ngpu_engine *>(e)->mu);
  return e->dict ? e->dict->dev.m : 0;
}

int ngpu_dict_probe(const ngpu_dict *d, const uint8_t *d_digests, uint64_t stride, uint64_t n,
                    ngpu_dict_hit *d_hits, void *stream) {
  if (!d || (n && (!d_digests || !d_hits)) || stride < 32 || (stride & 15)) return NGPU_EINVAL;
  if (!d->parts.empty()) return NGPU_EINVAL;  // node dicts are probed through an engine
  DeviceGuard dg(d->device);
  launch_dict_probe(d_digests, stride, n, d->dev, d_hits, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : NGPU_EHIP;
}

// Routing for dicts partitioned across processes (nydus_gpu/dist.py): the
// owner bucketing runs here, in two kernels, instead of an argsort / bincount /
// gather in PyTorch.  Runs on the device of the caller's current context.
int ngpu_route_digests(const uint8_t *d_digests, uint64_t stride, uint64_t n, uint32_t world,
                       uint64_t seg_cap, uint32_t rounds, uint8_t *d_out, uint32_t *d_rows,
                       uint32_t *d_counts, void *stream) {
  if (!world || world > 64 || !d_counts || (n && (!d_digests || !d_out || !d_rows)) ||
      stride < 32 || (stride & 15) || n >= 0xFFFFFFFFull)
    return NGPU_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (seg_cap) {
    const uint64_t slots = (uint64_t)rounds * world * seg_cap;
    if ((uint64_t)rounds * seg_cap < n) return NGPU_EINVAL;
    if (hipMemsetAsync(d_out, 0, slots * 32, s) != hipSuccess ||
        hipMemsetAsync(d_rows, 0xFF, slots * 4, s) != hipSuccess)
      return NGPU_EHIP;
  }
  launch_route(d_digests, stride, n, world, seg_cap, d_counts, d_out, d_rows, s);
  return hipGetLastError() == hipSuccess ? 0 : NGPU_EHIP;
}

int ngpu_route_hits(const ngpu_dict_hit *d_routed, const uint32_t *d_rows, uint64_t m,
                    ngpu_dict_hit *d_hits, void *stream) {
  if (m && (!d_routed || !d_rows || !d_hits)) return NGPU_EINVAL;
  launch_hits_scatter(d_routed, d_rows, m, d_hits, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : NGPU_EHIP;
}

int ngpu_dict_probe_device(ngpu_engine *e, const uint8_t *d_digests, uint64_t stride,
                           uint64_t n, ngpu_dict_hit *d_hits, void *stream) {
  if (!e || (n && (!d_digests || !d_hits)) || stride < 32 || (stride & 15))
    return NGPU_EINVAL;
  std::lock_guard<std::mutex> g(e->mu);
  DeviceGuard dg(e->device);
  launch_dict_probe(d_digests, stride, n, e->dict ? e->dict->dev : DictDevice{}, d_hits,
                    (hipStream_t)stream);
  HIP_TRY(e, hipGetLastError());
  return 0;
}

}  // extern "C"
