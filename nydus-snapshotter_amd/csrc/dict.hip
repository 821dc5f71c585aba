// dict.hip — chunk dicts (PackOption.ChunkDictPath, builder.go:122-124) as
// reference-counted HBM objects, and their C ABI (include/nydus_gpu.h).
//
// The reference hands `--chunk-dict bootstrap=P` to every nydus-image process
// it spawns; each loads its own HashChunkDict ([nydus v2.3.0]
// builder/src/core/chunk_dict.rs, external, VERIFY).  Here one load serves
// every Pack that names the same unchanged file (the engine's open cache),
// and a Pack pins the dict it was opened with, so packs against different
// dicts can be open on one engine at once.
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
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>

#include "blob.hpp"
#include "dict_fold_plan.hpp"
#include "dict_grow_plan.hpp"
#include "dict_retire_plan.hpp"
#include "engine_internal.hpp"
#include "host_window.hpp"

using namespace ngpu;

extern "C" const char *ngpu_host_error(void);

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
static int storage_alloc(ngpu_engine *e, uint64_t rec_cap, uint64_t table_cap, bool place,
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
static void dict_bind(ngpu_dict *d, uint64_t m, uint32_t n_blobs) {
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

namespace {

// A dict build runs on a stream of its own, outside the engine lock: a load
// of a 200M-entry bootstrap takes seconds, and under e->mu (round 3) it stalled
// every Pack of the engine for that long, while its stream syncs on the
// engine's own stream waited for their work too.
struct BuildStream {
  hipStream_t s = nullptr;
  explicit BuildStream(int device) {
    DeviceGuard g(device);
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      s = nullptr;
    }
  }
  ~BuildStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

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
  for (uint64_t i = 0; i < m; ++i) {
    const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
    nb = std::max(nb, r->blob_index + 1);
  }
  if (n_blobs) {
    if (nb > n_blobs)
      return fail(e, NGPU_EFORMAT, "chunk dict record points at blob %u of %u", nb - 1, n_blobs);
    nb = n_blobs;
  }
  if (nb > (1u << 20)) return fail(e, NGPU_EINVAL, "chunk dict blob index %u too large", nb - 1);
  ngpu_dict *d = dict_new(e);
  int rc = dict_alloc(e, d, m, nb, true);
  if (rc) {
    dict_unref(d);
    return rc;
  }
  for (uint64_t i = 0; i < m; ++i) {
    const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
    d->st->place[i] = DictPlace{r->compressed_offset, r->compressed_size, r->flags};
  }
  if (blobs && n_blobs) d->blob_table.assign(blobs, blobs + 256ull * n_blobs);
  // upload in batches of <= 1M records, unpack to dict records on the GPU
  const uint64_t batch = std::min<uint64_t>(m, 1u << 20);
  uint8_t *tmp = nullptr;
  uint32_t *tmp_gid = nullptr;
  if (m && (hipMalloc((void **)&tmp, batch * 80) != hipSuccess ||
            (gids && hipMalloc((void **)&tmp_gid, batch * 4) != hipSuccess))) {
    if (tmp) (void)hipFree(tmp);
    dict_unref(d);
    return fail(e, NGPU_ENOMEM, "chunk dict: staging allocation failed");
  }
  DictRec *rec = const_cast<DictRec *>(d->dev.rec);
  for (uint64_t a = 0; a < m && !rc; a += batch) {
    const uint64_t k = std::min(batch, m - a);
    if (hipMemcpyAsync(tmp, recs + 80 * a, k * 80, hipMemcpyHostToDevice, bs.s) != hipSuccess ||
        (gids && hipMemcpyAsync(tmp_gid, gids + a, k * 4, hipMemcpyHostToDevice, bs.s) !=
                     hipSuccess)) {
      rc = fail(e, NGPU_EHIP, "chunk dict: upload failed");
      break;
    }
    launch_dict_unpack(tmp, k, gids ? tmp_gid : nullptr, (uint32_t)a, rec + a, bs.s);
    // the next batch overwrites tmp
    if (hipStreamSynchronize(bs.s) != hipSuccess) rc = fail(e, NGPU_EHIP, "chunk dict: unpack failed");
  }
  if (tmp_gid) (void)hipFree(tmp_gid);
  if (tmp) (void)hipFree(tmp);
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
    launch_dict_pack(dg, us, bl, ix, uo, gid, m, rec, bs.s);
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
  for (uint64_t i = 0; i < k; ++i) {
    const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
    if (n_blobs && r->blob_index >= n_blobs)
      return fail(e, NGPU_EFORMAT, "chunk dict record points at blob %u of %u", r->blob_index,
                  n_blobs);
    if (r->blob_index >= (1u << 20))
      return fail(e, NGPU_EINVAL, "chunk dict blob index %u too large", r->blob_index);
    nb = std::max(nb, r->blob_index + 1);
  }
  if (n_blobs) nb = n_blobs;
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
    const uint64_t batch = std::min<uint64_t>(k, 1u << 20);
    uint8_t *tmp = nullptr;
    uint32_t *tmp_gid = nullptr;
    if (!bs) {
      rc = fail(e, NGPU_EHIP, "chunk dict: no build stream");
    } else if (staged && (hipMalloc((void **)&tmp, batch * 80) != hipSuccess ||
                          (gids && hipMalloc((void **)&tmp_gid, batch * 4) != hipSuccess))) {
      (void)hipGetLastError();
      rc = fail(e, NGPU_ENOMEM, "chunk dict: staging allocation failed");
    }
    // NGPU_DICT_TRACE=1: one stderr line per extend with its device time -- an
    // in-place append from before its first launch (after the records' upload)
    // to the end of the inserts, a copy from before the device-to-device copy to
    // the end of the table build (tools/dict_extend_bench.py reads it); off: no
    // event is made
    static const bool trace = [] {
      const char *v = getenv("NGPU_DICT_TRACE");
      return v && v[0] == '1';
    }();
    hipEvent_t tev[2] = {};
    if (!rc && trace)
      for (hipEvent_t &x : tev)
        if (hipEventCreate(&x) != hipSuccess) x = nullptr;
    if (!share && tev[0] && tev[1]) (void)hipEventRecord(tev[0], bs);
    if (!rc && !share && m &&
        hipMemcpyAsync(dst->rec, st->rec, m * sizeof(DictRec), hipMemcpyDeviceToDevice, bs) !=
            hipSuccess)
      rc = fail(e, NGPU_EHIP, "chunk dict: copy of the base's records failed");
    if (!rc && want_place) {
      if (!share && base->has_place) memcpy(dst->place, st->place, m * sizeof(DictPlace));
      if (!staged) {
        if (src.rows) memcpy(dst->place + m, src.rows, k * sizeof(DictPlace));
      } else {
        for (uint64_t i = 0; i < k; ++i) {
          const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
          dst->place[m + i] = DictPlace{r->compressed_offset, r->compressed_size, r->flags};
        }
      }
    }
    // launch 1 (per batch of <= 1M records): rec[m + a ..) from the 80-B records
    for (uint64_t a = 0; staged && a < k && !rc; a += batch) {
      const uint64_t c = std::min(batch, k - a);
      if (hipMemcpyAsync(tmp, recs + 80 * a, c * 80, hipMemcpyHostToDevice, bs) != hipSuccess ||
          (gids && hipMemcpyAsync(tmp_gid, gids + a, c * 4, hipMemcpyHostToDevice, bs) !=
                       hipSuccess)) {
        rc = fail(e, NGPU_EHIP, "chunk dict: upload failed");
        break;
      }
      if (share && a == 0 && tev[0] && tev[1]) (void)hipEventRecord(tev[0], bs);
      launch_dict_unpack(tmp, c, gids ? tmp_gid : nullptr, (uint32_t)(m + a), dst->rec + m + a, bs,
                         src.blob0);
      // the next batch overwrites tmp (one batch: the sync after the inserts serves)
      if (a + c < k && hipStreamSynchronize(bs) != hipSuccess)
        rc = fail(e, NGPU_EHIP, "chunk dict: unpack failed");
    }
    // (device source) launch 1: its own kernel writes rec[m, m + k)
    if (!staged && !rc) {
      if (share && tev[0] && tev[1]) (void)hipEventRecord(tev[0], bs);
      src.write(src, dst->rec + m, m, bs);
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
    if (tev[0] && tev[1]) (void)hipEventRecord(tev[1], bs);
    if (bs && hipStreamSynchronize(bs) != hipSuccess && !rc)
      rc = fail(e, NGPU_EHIP, "chunk dict: extend failed");
    if (tev[0] && tev[1]) {
      float ms = 0;
      if (!rc && hipEventElapsedTime(&ms, tev[0], tev[1]) == hipSuccess) {
        if (staged)
          fprintf(stderr, "ngpu dict_extend %s m=%llu k=%llu device_us=%.1f\n", share ? "share" : "fork",
                  (unsigned long long)m, (unsigned long long)k, ms * 1000.0);
        else  // the fold's keep + scan ran before the counts came back
          fprintf(stderr, "ngpu %s %s m=%llu k=%llu n=%llu device_us=%.1f keep_scan_us=%.1f\n", src.name,
                  share ? "share" : "fork", (unsigned long long)m, (unsigned long long)k,
                  (unsigned long long)src.n, ms * 1000.0 + src.pre_us, src.pre_us);
      }
    }
    for (hipEvent_t x : tev)
      if (x) (void)hipEventDestroy(x);
    if (tmp_gid) (void)hipFree(tmp_gid);
    if (tmp) (void)hipFree(tmp);
  }
  if (rc) {
    storage_unref(dst);
    return rc;
  }
  ngpu_dict *d = new ngpu_dict();
  d->device = base->device;
  d->digester = base->digester;
  d->chunk_size = base->chunk_size;
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
    st = new DictStorage();
    st->device = e->device;
    st->rec_cap = cap;
    st->table_cap = ~0ull;
    st->used = m + k;
    if (cap && !(st->place = (DictPlace *)malloc(cap * sizeof(DictPlace)))) {
      delete st;
      return fail(e, NGPU_ENOMEM, "chunk dict: no host memory for %llu placement rows",
                  (unsigned long long)cap);
    }
    if (base_rows) memcpy(st->place, base->st->place, m * sizeof(DictPlace));
  }
  if (!recs && k) memcpy(st->place + m, rows, k * sizeof(DictPlace));
  for (uint64_t i = 0; recs && i < k; ++i) {
    const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(recs + 80 * i);
    st->place[m + i] = DictPlace{r->compressed_offset, r->compressed_size, r->flags};
  }
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

int dict_retire_records(ngpu_engine *e, const ngpu_dict *base, const std::vector<uint32_t> &bitmap,
                        const std::vector<uint32_t> &remap, uint32_t nb, const DictPlace *place,
                        DictKeep *keep, ngpu_dict **out) {
  DeviceGuard dg(e->device);
  const uint64_t m = base->dev.m;
  const uint32_t nb0 = base->dev.n_blobs;
  const uint64_t nw = (m + 63) / 64, nt = dict_retire_scan_tiles(m);
  BuildStream bs(e->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  // one scratch allocation: keep words, tile sums (+ the total), word counts /
  // prefixes, the retire bitmap and the blob remap
  const uint64_t o_sums = 8 * nw, o_cnt = o_sums + 8 * (nt + 1), o_bits = o_cnt + 4 * nw,
                 o_remap = o_bits + 4 * bitmap.size(), bytes = o_remap + 4 * remap.size();
  uint8_t *scr = nullptr;
  if (hipMalloc((void **)&scr, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, NGPU_ENOMEM, "dict retire: scratch allocation failed");
  }
  uint64_t *d_words = (uint64_t *)scr, *d_sums = (uint64_t *)(scr + o_sums);
  uint32_t *d_cnt = (uint32_t *)(scr + o_cnt), *d_bits = (uint32_t *)(scr + o_bits),
           *d_remap = (uint32_t *)(scr + o_remap);
  // NGPU_DICT_TRACE=1: one stderr line per retire with its device time, launches
  // 1-2 plus launches 3-4 (the allocation between them is host time)
  static const bool trace = [] {
    const char *v = getenv("NGPU_DICT_TRACE");
    return v && v[0] == '1';
  }();
  hipEvent_t tev[4] = {};
  bool timed = trace;
  if (trace)
    for (hipEvent_t &x : tev)
      if (hipEventCreate(&x) != hipSuccess) x = nullptr, timed = false;
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
    if (timed) (void)hipEventRecord(tev[0], bs.s);
    launch_dict_keep_scan(base->st ? base->st->rec : nullptr, m, d_bits, nb0, d_words, d_cnt, d_sums,
                          bs.s);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "dict retire: keep scan failed");
    if (timed) (void)hipEventRecord(tev[1], bs.s);
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
  if (!rc && s > m) rc = fail(e, NGPU_EHIP, "dict retire: %llu survivors of %llu records",
                              (unsigned long long)s, (unsigned long long)m);
  if (!rc)
    rc = storage_alloc(e, dict_retire_rec_cap(s), dict_retire_table_cap(s), place && s, &dst);
  if (!rc) {
    dst->used = s;
    if (timed) (void)hipEventRecord(tev[2], bs.s);
    launch_dict_compact(base->st ? base->st->rec : nullptr, m, d_words, d_cnt, d_remap, nb0, dst->rec,
                        s, bs.s);
    launch_dict_build(dst->rec, s, dst->table, dst->table_cap, bs.s);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "dict retire: compaction failed");
    if (timed) (void)hipEventRecord(tev[3], bs.s);
  }
  // the placement rows, while the device moves the records
  if (!rc && place && s) dict_retire_place(hk, m, place, dst->place, s);
  if (hipStreamSynchronize(bs.s) != hipSuccess && !rc)
    rc = fail(e, NGPU_EHIP, "dict retire: compaction failed");
  if (timed) {
    float a = 0, b = 0;
    if (!rc && hipEventElapsedTime(&a, tev[0], tev[1]) == hipSuccess &&
        hipEventElapsedTime(&b, tev[2], tev[3]) == hipSuccess)
      fprintf(stderr, "ngpu dict_retire m=%llu s=%llu device_us=%.1f keep_scan_us=%.1f compact_build_us=%.1f\n",
              (unsigned long long)m, (unsigned long long)s, (a + b) * 1000.0, a * 1000.0, b * 1000.0);
  }
  for (hipEvent_t x : tev)
    if (x) (void)hipEventDestroy(x);
  (void)hipFree(scr);
  if (rc) {
    storage_unref(dst);
    return rc;
  }
  ngpu_dict *d = new ngpu_dict();
  d->device = base->device;
  d->digester = base->digester;
  d->chunk_size = base->chunk_size;
  d->st = dst;
  d->has_place = place && s;
  dict_bind(d, s, nb);
  *out = d;
  return 0;
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
    for (uint64_t i = 0; i < c; ++i) {
      const DictRec &r = h[i];
      RafsV6ChunkInfo x;
      memset(&x, 0, sizeof x);
      memcpy(x.block_id, r.digest, 32);
      x.blob_index = r.blob;
      x.uncompressed_size = r.usize;
      x.uncompressed_offset = r.uoff;
      x.index = r.index;
      if (rows) {
        x.compressed_offset = rows[a + i].compressed_offset;
        x.compressed_size = rows[a + i].compressed_size;
        x.flags = rows[a + i].flags;
      } else {  // as ngpu_dict_load documents: stored uncompressed at offset 0
        x.compressed_size = r.usize;
      }
      memcpy(records + 80 * (a + i), &x, 80);
    }
  }
  return 0;
}

namespace {

// RafsSuperFlags HASH_SHA256 (0x8) -> sha256, else blake3 ([nydus v2.3.0]
// RafsSuperMeta::get_digester, VERIFY; the fixture's ext flags are 0x6).
uint32_t digester_of_flags(uint64_t f) { return (f & 0x8) ? NGPU_DIGEST_SHA256 : NGPU_DIGEST_BLAKE3; }

int read_at(FILE *f, void *buf, uint64_t n, uint64_t off) {
  if (!n) return 0;
  if (fseeko(f, (off_t)off, SEEK_SET) != 0 || fread(buf, 1, n, f) != n) return -1;
  return 0;
}

}  // namespace

namespace {

// A RAFS v5 chunk-dict bootstrap (FsVersion "5" with ChunkDictPath): parsed
// by the host code (parse_v5_bootstrap, blob.cpp), checked against the engine.
int parse_v5_dict(ngpu_engine *e, const char *path, const std::vector<uint8_t> &b,
                  std::vector<uint8_t> *recs_out, std::vector<uint8_t> *blobs_out) {
  uint32_t dg = 0, bs = 0;
  if (int rc = parse_v5_bootstrap(b.data(), b.size(), &dg, &bs, recs_out, blobs_out))
    return fail(e, rc, "chunk dict %s: %s", path, ngpu_host_error());
  if (dg != e->cfg.digester)
    return fail(e, NGPU_EINVAL, "chunk dict %s: inconsistent digester %s vs %s", path,
                dg ? "sha256" : "blake3", e->cfg.digester ? "sha256" : "blake3");
  if (bs != e->cfg.chunk_size)
    return fail(e, NGPU_EINVAL, "chunk dict %s: inconsistent chunk size 0x%x vs 0x%x", path, bs,
                e->cfg.chunk_size);
  return 0;
}

}  // namespace

// Parse + check a chunk-dict bootstrap against engine e's options: its chunk
// records (80 B each) and blob table (256 B each).  RAFS v6 for a FsVersion
// 6 engine, RAFS v5 for FsVersion 5; the other pairings are nydus-image's
// "inconsistent RAFS version" error.
int read_dict_bootstrap(ngpu_engine *e, const char *path, uint64_t file_size,
                        std::vector<uint8_t> *recs_out, std::vector<uint8_t> *blobs_out,
                        uint64_t *table_at) {
  FILE *f = fopen(path, "rb");
  if (!f) return fail(e, NGPU_EIO, "open chunk dict %s", path);
  uint8_t sb[kRafsV6ExtSuperBlockOffset + 256];
  uint32_t magic = 0, magic5 = 0, ver5 = 0;
  const bool got_sb = file_size >= sizeof sb && read_at(f, sb, sizeof sb, 0) == 0;
  if (got_sb) {
    memcpy(&magic, sb + kRafsV6SuperBlockOffset, 4);
    memcpy(&magic5, sb, 4);
    memcpy(&ver5, sb + 4, 4);
  }
  const bool v6 = got_sb && magic == kRafsV6Magic;
  const bool v5 = got_sb && magic5 == kRafsV5Magic && ver5 == kRafsV5Version;
  if (!v5 && !v6) {
    fclose(f);
    return fail(e, NGPU_EFORMAT, "chunk dict %s is not a RAFS v5/v6 bootstrap", path);
  }
  if ((v6 ? 6u : 5u) != e->cfg.fs_version) {
    fclose(f);
    return fail(e, NGPU_EINVAL,
                "chunk dict %s: RAFS v%d bootstrap for a FsVersion %u engine (inconsistent version)",
                path, v6 ? 6 : 5, e->cfg.fs_version);
  }
  if (v5) {
    std::vector<uint8_t> all(file_size);
    const int r = read_at(f, all.data(), file_size, 0);
    fclose(f);
    if (r) return fail(e, NGPU_EIO, "chunk dict %s: short read", path);
    return parse_v5_dict(e, path, all, recs_out, blobs_out);
  }
  const uint8_t *x = sb + kRafsV6ExtSuperBlockOffset;
  uint64_t flags, bto, cto, cts;
  uint32_t bts, cs;
  memcpy(&flags, x, 8);
  memcpy(&bto, x + 8, 8);
  memcpy(&bts, x + 16, 4);
  memcpy(&cs, x + 20, 4);
  memcpy(&cto, x + 24, 8);  // RafsV6ChunkInfoOffset = 1024+128+24 (layout.go:27)
  memcpy(&cts, x + 32, 8);
  const uint32_t dg = digester_of_flags(flags);
  int rc = 0;
  if (dg != e->cfg.digester)
    rc = fail(e, NGPU_EINVAL, "chunk dict %s: inconsistent digester %s vs %s", path,
              dg ? "sha256" : "blake3", e->cfg.digester ? "sha256" : "blake3");
  else if (cs != e->cfg.chunk_size)
    rc = fail(e, NGPU_EINVAL, "chunk dict %s: inconsistent chunk size 0x%x vs 0x%x", path, cs,
              e->cfg.chunk_size);
  else if (cts % 80 || bts % 256 || cto > file_size || cts > file_size - cto || bto > file_size ||
           bts > file_size - bto)
    rc = fail(e, NGPU_EFORMAT, "chunk dict %s: bad chunk/blob table bounds", path);
  if (!rc && table_at) {  // v6, records left in the file: the caller streams them
    table_at[0] = cto;
    table_at[1] = cts;
    recs_out->clear();
    blobs_out->resize(bts);
    if (read_at(f, blobs_out->data(), bts, bto) != 0)
      rc = fail(e, NGPU_EIO, "chunk dict %s: short read", path);
  } else if (!rc) {
    recs_out->resize(cts);
    blobs_out->resize(bts);
    if (read_at(f, recs_out->data(), cts, cto) != 0 || read_at(f, blobs_out->data(), bts, bto) != 0)
      rc = fail(e, NGPU_EIO, "chunk dict %s: short read", path);
  }
  fclose(f);
  return rc;
}

namespace {

// A RAFS v6 chunk table streamed from the file into HBM:
// 1M-record pieces (80 MB) go through three pinned buffers; kReadThreads host
// threads pread a piece (page cache or disk) and scan it (blob index bound,
// the compressed placements the blob writer keeps on the host) while the
// previous pieces cross PCIe and the unpack kernel turns them into dict
// records, so the file read, the H2D copy and the unpack overlap instead of
// following one another over the whole table.  Same records, same table
// order, same checks as dict_from_records.
constexpr uint64_t kStreamPiece = 1u << 20;      // records per piece
constexpr uint64_t kStreamMinBytes = 256u << 20;  // smaller tables: one read, dict_from_records
constexpr int kReadThreads = 8;

int pread_full(int fd, uint8_t *dst, uint64_t n, uint64_t off) {
  while (n) {
    const ssize_t r = pread(fd, dst, n, (off_t)off);
    if (r <= 0) {
      if (r < 0 && errno == EINTR) continue;
      return -1;
    }
    dst += r, n -= (uint64_t)r, off += (uint64_t)r;
  }
  return 0;
}

int dict_stream_v6(ngpu_engine *e, const char *path, uint64_t cto, uint64_t m,
                   const std::vector<uint8_t> &blobs, ngpu_dict **out) {
  DeviceGuard dg(e->device);
  BuildStream bs(e->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "chunk dict: no build stream");
  if (m >= 0xFFFFFFFFull)
    return fail(e, NGPU_EINVAL, "chunk dict too large (%llu entries)", (unsigned long long)m);
  const uint32_t n_blobs = (uint32_t)(blobs.size() / 256);
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return fail(e, NGPU_EIO, "open chunk dict %s", path);
  ngpu_dict *d = dict_new(e);
  uint8_t *pin[3] = {}, *tmp[2] = {};
  hipEvent_t ev[3] = {};
  int rc = dict_alloc(e, d, m, n_blobs, true);
  for (int i = 0; i < 3 && !rc; ++i)
    if (hipHostMalloc((void **)&pin[i], kStreamPiece * 80, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess)
      rc = fail(e, NGPU_ENOMEM, "chunk dict: pinned staging allocation failed");
  for (int i = 0; i < 2 && !rc; ++i)
    if (hipMalloc((void **)&tmp[i], kStreamPiece * 80) != hipSuccess)
      rc = fail(e, NGPU_ENOMEM, "chunk dict: staging allocation failed");
  if (!rc && n_blobs) d->blob_table.assign(blobs.begin(), blobs.end());
  DictRec *rec = const_cast<DictRec *>(d->dev.rec);
  uint32_t nb = 0;
  for (uint64_t a = 0, k = 0; a < m && !rc; a += kStreamPiece, ++k) {
    const uint64_t cnt = std::min(kStreamPiece, m - a);
    uint8_t *h = pin[k % 3];
    if (k >= 3 && hipEventSynchronize(ev[k % 3]) != hipSuccess) {  // its last copy is done
      rc = fail(e, NGPU_EHIP, "chunk dict: upload failed");
      break;
    }
    // read + scan the piece on kReadThreads threads (disjoint record ranges)
    std::atomic<int> bad{0};
    uint32_t tnb[kReadThreads] = {};
    std::vector<std::thread> th;
    const uint64_t per = (cnt + kReadThreads - 1) / kReadThreads;
    for (int t = 0; t < kReadThreads; ++t) {
      const uint64_t r0 = std::min(cnt, per * t), r1 = std::min(cnt, per * (t + 1));
      if (r0 == r1) continue;
      th.emplace_back([&, r0, r1, t] {
        if (pread_full(fd, h + 80 * r0, 80 * (r1 - r0), cto + 80 * (a + r0))) {
          bad = 1;
          return;
        }
        uint32_t x = 0;
        for (uint64_t i = r0; i < r1; ++i) {
          const RafsV6ChunkInfo *r = reinterpret_cast<const RafsV6ChunkInfo *>(h + 80 * i);
          x = std::max(x, r->blob_index + 1);
          d->st->place[a + i] = DictPlace{r->compressed_offset, r->compressed_size, r->flags};
        }
        tnb[t] = x;
      });
    }
    for (auto &x : th) x.join();
    for (uint32_t x : tnb) nb = std::max(nb, x);
    if (bad) {
      rc = fail(e, NGPU_EIO, "chunk dict %s: short read", path);
      break;
    }
    if (hipMemcpyAsync(tmp[k % 2], h, cnt * 80, hipMemcpyHostToDevice, bs.s) != hipSuccess) {
      rc = fail(e, NGPU_EHIP, "chunk dict: upload failed");
      break;
    }
    launch_dict_unpack(tmp[k % 2], cnt, nullptr, (uint32_t)a, rec + a, bs.s);
    if (hipEventRecord(ev[k % 3], bs.s) != hipSuccess) rc = fail(e, NGPU_EHIP, "chunk dict: unpack failed");
  }
  close(fd);
  if (!rc && hipStreamSynchronize(bs.s) != hipSuccess) rc = fail(e, NGPU_EHIP, "chunk dict: unpack failed");
  if (rc) (void)hipStreamSynchronize(bs.s);
  for (uint8_t *x : tmp)
    if (x) (void)hipFree(x);
  for (int i = 0; i < 3; ++i) {
    if (pin[i]) (void)hipHostFree(pin[i]);
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  }
  if (!rc && n_blobs && nb > n_blobs)
    rc = fail(e, NGPU_EFORMAT, "chunk dict record points at blob %u of %u", nb - 1, n_blobs);
  if (!rc && nb > (1u << 20)) rc = fail(e, NGPU_EINVAL, "chunk dict blob index %u too large", nb - 1);
  if (!rc && !n_blobs) d->dev.n_blobs = nb;
  if (!rc) rc = dict_build(e, d, bs.s);
  if (rc) {
    dict_unref(d);
    return rc;
  }
  *out = d;
  return 0;
}

// Parse + check + load a RAFS v5/v6 chunk-dict bootstrap (no engine lock).
int dict_load_file(ngpu_engine *e, const char *path, const struct stat &st, ngpu_dict **out) {
  std::vector<uint8_t> recs, blobs;
  uint64_t table[2] = {0, 0};
  int rc = read_dict_bootstrap(e, path, (uint64_t)st.st_size, &recs, &blobs, table);
  if (rc) return rc;
  ngpu_dict *d = nullptr;
  if (table[1] >= kStreamMinBytes) {  // v6 and large: stream it
    if ((rc = dict_stream_v6(e, path, table[0], table[1] / 80, blobs, &d))) return rc;
  } else {
    if (table[1]) {  // v6, small: one read
      recs.resize(table[1]);
      FILE *f = fopen(path, "rb");
      rc = (!f || read_at(f, recs.data(), table[1], table[0]))
               ? fail(e, NGPU_EIO, "chunk dict %s: short read", path)
               : 0;
      if (f) fclose(f);
      if (rc) return rc;
    }
    if ((rc = dict_from_records(e, recs.data(), recs.size() / 80, blobs.data(), blobs.size() / 256,
                                &d, nullptr)))
      return rc;
  }
  d->path = path;
  d->st_dev = st.st_dev;
  d->st_ino = st.st_ino;
  d->st_size = st.st_size;
  d->st_mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000 + st.st_mtim.tv_nsec;
  *out = d;
  return 0;
}

constexpr size_t kDictCache = 4;

}  // namespace
}  // namespace ngpu

extern "C" {

static int dict_open(ngpu_engine *e, const char *path, ngpu_dict **out);

int ngpu_dict_open(ngpu_engine *e, const char *path, ngpu_dict **out) {
  return guarded([&] { return dict_open(e, path, out); });
}

static bool same_file(const ngpu_dict *d, const char *path, const struct stat &st, int64_t mt) {
  return d->path == path && d->st_dev == (uint64_t)st.st_dev && d->st_ino == (uint64_t)st.st_ino &&
         d->st_size == (uint64_t)st.st_size && d->st_mtime_ns == mt;
}

// The engine lock covers only the cache lookups and the insert: the bootstrap
// is read, parsed and built in HBM without it, and dicts leaving the cache are
// released after it is dropped (the last release hipFrees, a device-wide wait).
// Two threads opening the same changed file may both load it; the second
// insert finds the first and drops its own copy.
static int dict_open(ngpu_engine *e, const char *path, ngpu_dict **out) {
  if (!e || !path || !out) return NGPU_EINVAL;
  *out = nullptr;
  struct stat st;
  if (stat(path, &st) != 0) return fail(e, NGPU_EIO, "stat chunk dict %s", path);
  const int64_t mt = (int64_t)st.st_mtim.tv_sec * 1000000000 + st.st_mtim.tv_nsec;
  std::vector<ngpu_dict *> drop;
  auto release_dropped = [&] {
    for (ngpu_dict *x : drop) dict_unref(x);
    drop.clear();
  };
  {
    std::lock_guard<std::mutex> g(e->mu);
    auto &c = e->dict_cache;
    for (size_t i = 0; i < c.size(); ++i) {
      ngpu_dict *d = c[i];
      if (d->path != path) continue;
      if (same_file(d, path, st, mt)) {
        dict_ref(d);
        *out = d;
        return 0;
      }
      c.erase(c.begin() + (long)i);  // the file changed: forget the old load
      drop.push_back(d);
      break;
    }
  }
  release_dropped();
  ngpu_dict *d = nullptr;
  if (int rc = dict_load_file(e, path, st, &d)) return rc;
  {
    std::lock_guard<std::mutex> g(e->mu);
    auto &c = e->dict_cache;
    for (ngpu_dict *x : c)
      if (same_file(x, path, st, mt)) {  // another thread loaded it meanwhile
        dict_ref(x);
        drop.push_back(d);
        d = x;
        break;
      }
    if (std::find(c.begin(), c.end(), d) == c.end()) {
      for (size_t i = 0; i < c.size(); ++i)
        if (c[i]->path == path) {  // an older load of the same path
          drop.push_back(c[i]);
          c.erase(c.begin() + (long)i);
          break;
        }
      if (c.size() >= kDictCache) {
        drop.push_back(c.front());
        c.erase(c.begin());
      }
      dict_ref(d);  // the cache's reference
      c.push_back(d);
    }
  }
  release_dropped();
  *out = d;
  return 0;
}

int ngpu_dict_create(ngpu_engine *e, const void *records, uint64_t n, const void *blob_table,
                     uint32_t n_blobs, ngpu_dict **out) {
  if (!e || !out || (n && !records) || (n_blobs && !blob_table)) return NGPU_EINVAL;
  *out = nullptr;
  return guarded([&] {
    return dict_from_records(e, (const uint8_t *)records, n, (const uint8_t *)blob_table, n_blobs,
                             out, nullptr);
  });
}

static int dict_extend(ngpu_engine *e, ngpu_dict *base, const uint8_t *recs, uint64_t n,
                       const uint8_t *blobs, uint32_t n_blobs, ngpu_dict **out) {
  if (!base->parts.empty())
    return fail(e, NGPU_EINVAL, "dict extend: a node dict is extended with ngpu_node_dict_extend");
  if (base->device != e->device)
    return fail(e, NGPU_EINVAL, "chunk dict lives on device %d, engine on %d", base->device,
                e->device);
  if (int rc = dict_check(e, base)) return rc;
  uint32_t nb = 0;
  bool with_table = false;
  if (int rc = dict_extend_check(e, base, recs, n, blobs, n_blobs, &nb, &with_table)) return rc;
  ngpu_dict *d = nullptr;
  if (int rc = dict_extend_records(e, base, recs, n, base->dev.n_blobs, nb, nullptr, true, &d))
    return rc;
  if (with_table) {
    d->blob_table = base->blob_table;
    if (blobs && n_blobs) d->blob_table.insert(d->blob_table.end(), blobs, blobs + 256ull * n_blobs);
  }
  *out = d;
  return 0;
}

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

int ngpu_dict_extend_bootstrap(ngpu_engine *e, ngpu_dict *base, const char *path, uint32_t flags,
                               ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !e || !out || !path) return NGPU_EINVAL;
  return guarded([&]() -> int {
    if (e->cfg.fs_version != 6)
      return fail(e, NGPU_EINVAL, "dict extend takes RAFS v6 bootstraps (FsVersion %u engine)",
                  e->cfg.fs_version);
    struct stat st;
    if (stat(path, &st) != 0) return fail(e, NGPU_EIO, "stat chunk dict %s", path);
    std::vector<uint8_t> recs, blobs;
    if (int rc = read_dict_bootstrap(e, path, (uint64_t)st.st_size, &recs, &blobs)) return rc;
    return dict_extend(e, base, recs.data(), recs.size() / 80, blobs.data(),
                       (uint32_t)(blobs.size() / 256), out);
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
  if (bytes > e->fold_scr_cap) {
    // (nothing of an earlier fold still runs: each is complete when it returns)
    if (e->fold_scr) (void)hipFree(e->fold_scr);
    e->fold_scr = nullptr;
    e->fold_scr_cap = 0;
    const uint64_t want = std::max<uint64_t>(bytes + bytes / 2, 1u << 16);
    if (hipMalloc((void **)&e->fold_scr, want) != hipSuccess) {
      (void)hipGetLastError();
      e->fold_scr = nullptr;
      return fail(e, NGPU_ENOMEM, "dict fold: scratch allocation failed");
    }
    e->fold_scr_cap = want;
  }
  return 0;
}

extern "C" {

namespace {
struct FoldArgs {
  const ngpu_result *res;
  const ngpu_chunk *chunks;
  uint64_t n;
  const uint64_t *words;
  const uint32_t *prefix;
  const uint64_t *lfirst;
  uint64_t L;
  const uint32_t *lrank;
  uint32_t blob0;
  uint64_t k;
};
void fold_write(const DictRowSource &src, DictRec *dst, uint64_t m, hipStream_t s) {
  const FoldArgs &a = *static_cast<const FoldArgs *>(src.arg);
  launch_fold_scatter(a.res, a.chunks, a.n, a.words, a.prefix, a.lfirst, a.L, a.lrank, a.blob0,
                      (uint32_t)m, dst, a.k, s);
}
struct PackArgs {
  const uint8_t *dg;
  const uint32_t *us, *bl, *ix;
  const uint64_t *uo;
  uint64_t n;
  uint32_t blob0;
};
void pack_write(const DictRowSource &src, DictRec *dst, uint64_t m, hipStream_t s) {
  const PackArgs &a = *static_cast<const PackArgs *>(src.arg);
  launch_dict_pack_at(a.dg, a.us, a.bl, a.ix, a.uo, a.n, a.blob0, (uint32_t)m, dst, s);
}
}  // namespace

static int dict_fold_base_check(ngpu_engine *e, const ngpu_dict *base, const char *what) {
  if (!base->parts.empty()) return fail(e, NGPU_EINVAL, "%s: node dicts are not supported", what);
  if (base->device != e->device)
    return fail(e, NGPU_EINVAL, "chunk dict lives on device %d, engine on %d", base->device,
                e->device);
  return dict_check(e, base);
}

static int dict_extend_device(ngpu_engine *e, ngpu_dict *base, const PackArgs &a, uint32_t n_blobs,
                              ngpu_dict **out) {
  if (int rc = dict_fold_base_check(e, base, "dict extend_device")) return rc;
  ngpu_dict *d = nullptr;
  if (a.n == 0) {  // a handle equal to base
    if (int rc = dict_extend_rows(e, base, DictRowSource{}, 0, base->dev.n_blobs, base->has_place, &d))
      return rc;
    d->blob_table = base->blob_table;
    *out = d;
    return 0;
  }
  uint32_t nb = 0;
  bool with_table = false;
  if (int rc = dict_extend_check_blobs(e, base, a.n, n_blobs, false, n_blobs, &nb, &with_table))
    return rc;
  if (base->has_place)
    return fail(e, NGPU_EINVAL,
                "dict extend_device: the base keeps compressed placements, device arrays carry none");
  std::lock_guard<std::mutex> lane(e->fold_mu);
  DeviceGuard dg(e->device);
  if (int rc = fold_lane(e, 0)) return rc;
  PackArgs args = a;
  args.blob0 = base->dev.n_blobs;
  DictRowSource src;
  src.write = pack_write;
  src.arg = &args;
  src.stream = e->fold_stream;
  src.name = "dict_extend_device";
  src.n = a.n;
  if (int rc = dict_extend_rows(e, base, src, a.n, nb, false, &d)) return rc;
  *out = d;
  return 0;
}

int ngpu_dict_extend_device(ngpu_engine *e, ngpu_dict *base, const uint8_t *d_digests,
                            const uint32_t *d_usize, const uint32_t *d_blob_index,
                            const uint32_t *d_chunk_index, const uint64_t *d_uoff, uint64_t n,
                            uint32_t n_blobs, uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !e || !out || (n && (!d_digests || !d_usize || !d_blob_index)) ||
      ((uintptr_t)d_digests & 15))
    return NGPU_EINVAL;
  return guarded([&] {
    return dict_extend_device(e, base, PackArgs{d_digests, d_usize, d_blob_index, d_chunk_index, d_uoff, n, 0},
                              n_blobs, out);
  });
}

static int dict_fold(ngpu_engine *e, ngpu_dict *base, const ngpu_result *d_res,
                     const ngpu_chunk *d_chunks, uint64_t n, const uint64_t *d_lfirst, uint64_t L,
                     const ngpu_dict_place *placements, uint64_t n_placements, const uint8_t *blobs,
                     uint32_t n_blobs, ngpu_dict **out) {
  if (int rc = dict_fold_base_check(e, base, "dict fold")) return rc;
  if (n >= kDictMaxEntries || L >= kDictMaxEntries)
    return fail(e, NGPU_EINVAL, "dict fold: %llu chunks in %llu layers in one call",
                (unsigned long long)n, (unsigned long long)L);
  if (L <= 1) d_lfirst = nullptr, L = 1;  // one layer of n chunks
  std::lock_guard<std::mutex> lane(e->fold_mu);
  DeviceGuard dg(e->device);
  // scratch: keep words, tile sums (+ the total), counters, word counts /
  // prefixes, layer ranks
  const uint64_t nw = (n + 63) / 64, nt = dict_retire_scan_tiles(n);
  const uint64_t o_sums = 8 * nw, o_ctr = o_sums + 8 * (nt + 1), o_cnt = o_ctr + 8 * kFoldCtrWords,
                 o_rank = o_cnt + 4 * nw, bytes = o_rank + 4 * L;
  if (int rc = fold_lane(e, bytes)) return rc;
  const hipStream_t s = e->fold_stream;
  uint8_t *scr = e->fold_scr;
  uint64_t *d_words = (uint64_t *)scr, *d_sums = (uint64_t *)(scr + o_sums),
           *d_ctr = (uint64_t *)(scr + o_ctr);
  uint32_t *d_cnt = (uint32_t *)(scr + o_cnt), *d_rank = (uint32_t *)(scr + o_rank);
  static const bool trace = [] {
    const char *v = getenv("NGPU_DICT_TRACE");
    return v && v[0] == '1';
  }();
  hipEvent_t tev[2] = {};
  if (trace)
    for (hipEvent_t &x : tev)
      if (hipEventCreate(&x) != hipSuccess) x = nullptr;
  const bool timed = tev[0] && tev[1];
  uint64_t ctr[kFoldCtrWords] = {};
  int rc = 0;
  if (hipMemsetAsync(d_ctr, 0, 8 * kFoldCtrWords, s) != hipSuccess)
    rc = fail(e, NGPU_EHIP, "dict fold: keep scan failed");
  if (!rc) {
    if (timed) (void)hipEventRecord(tev[0], s);
    launch_fold_keep_scan(d_res, d_chunks, n, e->cfg.chunk_size, d_lfirst, L, d_words, d_cnt, d_sums,
                          d_rank, d_ctr, s);
    if (hipGetLastError() != hipSuccess) rc = fail(e, NGPU_EHIP, "dict fold: keep scan failed");
    if (timed) (void)hipEventRecord(tev[1], s);
  }
  // k, b and the refusals in one small copy: the call's only mid-way sync
  if (!rc && (hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipStreamSynchronize(s) != hipSuccess))
    rc = fail(e, NGPU_EHIP, "dict fold: keep scan failed");
  float pre_ms = 0;
  if (!rc && timed && hipEventElapsedTime(&pre_ms, tev[0], tev[1]) != hipSuccess) pre_ms = 0;
  for (hipEvent_t x : tev)
    if (x) (void)hipEventDestroy(x);
  if (rc) return rc;
  const uint64_t k = ctr[kFoldK], b = ctr[kFoldBlobs];
  // every check below comes before `used` is reserved or a storage byte is written
  if (ctr[kFoldBadLayer1])
    return fail(e, NGPU_EINVAL,
                "dict fold: layer_first is not 0 = first[0] <= ... <= first[%llu] = %llu at layer %llu",
                (unsigned long long)L, (unsigned long long)n,
                (unsigned long long)~ctr[kFoldBadLayer1]);
  if (ctr[kFoldBadKind])
    return fail(e, NGPU_EINVAL,
                "dict fold: chunk %llu is no dedup result (its kind is none of NEW / INTRA / DICT; "
                "%llu such chunks)",
                (unsigned long long)~ctr[kFoldBadKind1], (unsigned long long)ctr[kFoldBadKind]);
  if (ctr[kFoldBadLen])
    return fail(e, NGPU_EINVAL,
                "dict fold: NEW chunk %llu has length 0 or more than chunk size 0x%x (%llu such chunks)",
                (unsigned long long)~ctr[kFoldBadLen1], e->cfg.chunk_size,
                (unsigned long long)ctr[kFoldBadLen]);
  if (k > n || b > L || b > k)
    return fail(e, NGPU_EHIP, "dict fold: %llu NEW chunks in %llu layers of %llu chunks",
                (unsigned long long)k, (unsigned long long)b, (unsigned long long)n);
  const DictFoldPlace pr =
      dict_fold_place_rule(base->dev.m, base->has_place, placements != nullptr, n_placements, k);
  if (pr == kPlaceCount)
    return fail(e, NGPU_EINVAL, "dict fold: %llu placements for %llu NEW chunks",
                (unsigned long long)n_placements, (unsigned long long)k);
  if (pr == kPlaceMissing)
    return fail(e, NGPU_EINVAL, "dict fold: the base keeps compressed placements, the call gives none");
  if (pr == kPlaceUnwanted)
    return fail(e, NGPU_EINVAL, "dict fold: the base keeps no compressed placements, the call gives some");
  if (blobs && n_blobs != b)
    return fail(e, NGPU_EINVAL, "dict fold: a blob table of %u rows for %llu layers with a NEW chunk",
                n_blobs, (unsigned long long)b);
  uint32_t nb = 0;
  bool with_table = false;
  if (int r = dict_extend_check_blobs(e, base, k, (uint32_t)b, blobs && n_blobs, n_blobs, &nb, &with_table))
    return r;
  ngpu_dict *d = nullptr;
  if (k == 0) {  // a handle equal to base
    rc = dict_extend_rows(e, base, DictRowSource{}, 0, base->dev.n_blobs, base->has_place, &d);
  } else {
    const FoldArgs args{d_res, d_chunks, n, d_words, d_cnt, d_lfirst, L, d_rank, base->dev.n_blobs, k};
    DictRowSource src;
    src.write = fold_write;
    src.arg = &args;
    src.rows = reinterpret_cast<const DictPlace *>(placements);
    src.stream = s;
    src.name = "dict_fold";
    src.pre_us = pre_ms * 1000.0f;
    src.n = n;
    rc = dict_extend_rows(e, base, src, k, nb, pr == kPlaceKept, &d);
  }
  if (rc) return rc;
  if (with_table) {
    d->blob_table = base->blob_table;
    if (blobs && n_blobs) d->blob_table.insert(d->blob_table.end(), blobs, blobs + 256ull * n_blobs);
  }
  *out = d;
  return 0;
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
    if (!base->parts.empty())
      return fail(e, NGPU_EINVAL, "dict retire: a node dict is retired with ngpu_node_dict_retire");
    if (base->device != e->device)
      return fail(e, NGPU_EINVAL, "chunk dict lives on device %d, engine on %d", base->device,
                  e->device);
    if (int rc = dict_check(e, base)) return rc;
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
