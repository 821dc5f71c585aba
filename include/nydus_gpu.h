/*
 * nydus_gpu.h — C ABI of the MI355X chunk digest + dedup engine
 * (libnydusgpu.so).  Plain pointers and sizes only; no C++ or torch types.
 *
 * What this boundary replaces:
 *   The reference hands the digest/dedup stage to an external process:
 *   pkg/converter/tool/builder.go:148-178 (tool.Pack) execs
 *   `nydus-image create --type tar-rafs [--chunk-dict bootstrap=P]
 *    [--chunk-size S] ...` (argv built at builder.go:78-146) over FIFOs set up
 *   by packFromTar (pkg/converter/convert_unix.go:443-539).  Inside that
 *   process, per chunk: RafsDigest::from_buf + Node::deduplicate_chunk
 *   ([nydus v2.3.0] utils/src/digest.rs, builder/src/core/node.rs).
 *   This library performs exactly that stage in-process on the GPU; the Go
 *   side binds it from a new pkg/gpu cgo package.
 *
 * Errors: every function returns 0 on success or a negative NGPU_E* code;
 * ngpu_last_error() gives the per-engine message (Go wraps both into an
 * `error`, as builder.go:169-175 wraps the process exit status).  No
 * exceptions cross the ABI.  A missing or unusable GPU is an error
 * (NGPU_ENODEV): there is no CPU fallback in this library.
 *
 * Threading: one engine per device serves any number of goroutines.  Calls
 * take the engine's lock only while they enqueue work.  Calls on distinct
 * streams use distinct HBM workspaces (NGPU_WS_SLOTS, default 4) and run side
 * by side on the GPU; calls on one stream are ordered by it.  Every pack has
 * its own compute stream and waits for it, and writes its blob stream,
 * outside the lock, so Packs of an image's layers proceed concurrently.  A
 * split-stage caller (ngpu_digest_device, then ngpu_dedup_device) keeps both
 * stages of a layer on one stream: the dedup stage reports the bad-descriptor
 * count of the digest stage that ran last on its workspace.
 *
 * Lifetimes: engines, chunk dicts and packs are reference counted.  A pack
 * holds its engine and the dict it was opened with until it ends (close,
 * finish or abort), so ngpu_destroy / ngpu_dict_release with packs still open
 * only drop the caller's reference; the memory goes when the last pack ends.
 */
#ifndef NYDUS_GPU_H
#define NYDUS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGPU_ABI_VERSION 7

/* PackOption.Digester (API extension; maps to nydus-image --digester). */
enum ngpu_digester { NGPU_DIGEST_BLAKE3 = 0, NGPU_DIGEST_SHA256 = 1 };

/* Per-chunk dedup outcome ([nydus v2.3.0] Node::deduplicate_chunk), and the
 * two states a record has around it. */
enum ngpu_kind {
  NGPU_NEW = 0,   /* first occurrence: new data in this layer's blob */
  NGPU_INTRA = 1, /* duplicate of an earlier NEW chunk of this layer */
  NGPU_DICT = 2,  /* found in the chunk dict (PackOption.ChunkDictPath) */
  /* Written by the digest stage next to each digest (ngpu_digest_device).  The
   * dedup stage takes only records marked so: a caller that supplies its own
   * digests to ngpu_dedup_* sets kind = NGPU_DIGESTED. */
  NGPU_DIGESTED = 3,
  /* Set by the dedup stage on a record that reached it without a digest (kind
   * not NGPU_DIGESTED, or an all-zero digest): the record takes no part in
   * dedup, and the call fails with NGPU_EDEVICE when its stats are read
   * (ngpu_device_status for calls that read none). */
  NGPU_UNHASHED = 4
};

enum ngpu_error {
  NGPU_OK = 0,
  NGPU_EINVAL = -1,    /* bad argument (e.g. ChunkSize not a power of two) */
  NGPU_EHIP = -2,      /* HIP runtime error */
  NGPU_ENOMEM = -3,    /* device or pinned allocation failed */
  NGPU_ETAR = -4,      /* malformed / truncated tar stream */
  NGPU_EUNSUPP = -5,   /* unsupported input (GNU sparse tar entry) */
  NGPU_ENODEV = -6,    /* no usable gfx950 device */
  NGPU_EIO = -7,       /* file I/O (chunk-dict bootstrap) */
  NGPU_EFORMAT = -8,   /* not a RAFS v6 bootstrap / bad chunk table */
  NGPU_ENOTFOUND = -9, /* entry not found in a nydus blob (ErrNotFound,
                          pkg/converter/types.go:33-35) */
  NGPU_ECANCELED = -10, /* cancelled through the pack's cancel flag (the
                          reference's ctx.Done() / PackOption.Timeout kill of
                          the builder, builder.go:153-174) */
  NGPU_EDEVICE = -11   /* a device-side check failed: a chunk reached the
                          dedup stage without its digest (NGPU_UNHASHED) */
};

typedef struct ngpu_engine ngpu_engine;

/* Mirrors the PackOption fields this stage consumes
 * (pkg/converter/types.go:58-90). */
typedef struct {
  int32_t device;         /* HIP device ordinal */
  uint32_t digester;      /* enum ngpu_digester (default blake3) */
  uint32_t chunk_size;    /* PackOption.ChunkSize: power of two in
                             [0x1000, 0x1000000] (types.go:76); 0 -> 0x100000 */
  uint32_t fs_version;    /* PackOption.FsVersion 5 or 6; 0 -> 6
                             (builder.go:79-81).  v6 aligns uncompressed
                             offsets of NEW chunks to 4 KiB (v5 with
                             NGPU_FLAG_ALIGNED_CHUNK). */
  uint64_t staging_bytes; /* pinned staging slot size for host-buffer calls;
                             0 -> 256 MiB (two slots are allocated) */
  uint32_t leaves_per_lane; /* BLAKE3 tuning: 1 KiB leaves hashed per lane
                               (1, 2, 4, 8 or 16); 0 -> auto */
  uint32_t flags;         /* NGPU_FLAG_* */
} ngpu_config;

/* ngpu_config.flags */
#define NGPU_FLAG_TIMING 0x1u /* record HIP events around each stage */
/* PackOption.AlignedChunk (types.go:73-74, `--aligned-chunk`, builder.go:131-133):
 * 4 KiB-align the uncompressed offsets of NEW chunks for RAFS v5 too (v6
 * always aligns). */
#define NGPU_FLAG_ALIGNED_CHUNK 0x2u
/* Tuning / tests: never take the small-call paths.  By default chunk planning
 * and the dedup stage of calls with <= 4096 chunks run in one fused workgroup
 * each, and BLAKE3 layers of <= 32K leaves (one leaf per lane) hash each
 * compression on a quad of lanes; this flag keeps the multi-kernel grid path
 * and one lane per leaf (same results). */
#define NGPU_FLAG_GRID_STAGES 0x4u
/* Packs whose whole layer fit one staging slot and that close at about the
 * same time on one engine share ONE digest + multi-layer dedup launch set
 * (round 5: containerd converting an image's small layers concurrently).
 * The first to close waits for the other packs that may still join -- open,
 * not OCIRef, and with no more than one staging slot of tar so far -- to
 * close too: BLAKE3 at most 250 us; SHA-256 2 ms, restarted by every pack
 * that joins, at most 12 ms after the first (a SHA-256 batch holds the GPU
 * for one 1 MiB chunk's chain, ~21 ms, whatever its size).  A pack that cannot
 * join (its layer outgrew one slot, an OCIRef pack, a pack closing without
 * chunks) stops being waited for at that moment.  This flag gives every pack
 * its own launches (A/B, or a caller whose packs must never wait for each
 * other).  Same results. */
#define NGPU_FLAG_NO_BATCH 0x8u
/* Tuning (benchmarks only): bits 8..10 = 1 + BLAKE3 load mode (0 plain loads
 * with the whole-leaf fast path, 1 non-temporal loads, 2 next-block prefetch,
 * 3 both, 5 plain loads without the fast path); 0 = library default.  Every
 * mode computes the same digests; other values (5, 7) are rejected with
 * NGPU_EINVAL. */
#define NGPU_FLAG_LOAD_MODE_SHIFT 8
/* Tuning (benchmarks only): bits 11..13 = 1 + SHA-256 kernel (0: one lane per
 * chunk with schedule/round waves, 1: two lanes per chunk, 2: one lane per
 * chunk, each wave schedules its own blocks, 4: two lanes, one chunk group per
 * workgroup, 5: two lanes, four groups per workgroup); 0 = library default
 * (by chunk count); other values are rejected (NGPU_EINVAL). */
#define NGPU_FLAG_SHA_MODE_SHIFT 11

/* The builder's exit status (builder.go:169-175) for work enqueued on a
 * caller's stream: errors of device-pointer calls that read no stats (stats == NULL,
 * ngpu_digest_device, the *_layers_device calls): synchronises every stream
 * the engine's workspaces were last used on, returns the first error any
 * stage recorded since the previous ngpu_device_status (NGPU_EINVAL for bad or
 * overlapping descriptors, NGPU_EDEVICE for unhashed chunks; message in
 * ngpu_last_error) and clears them.  0: no stage recorded an error. */
int ngpu_device_status(ngpu_engine *eng);

/* Per-stage device time of the last process call (NGPU_FLAG_TIMING). */
typedef struct {
  float digest_ms;   /* leaf/group digest kernel (b3_groups / b3_quad_leaves /
                        sha256_*); BLAKE3: from the end of chunk planning, i.e.
                        the kernel plus its dispatch */
  float tree_ms;     /* BLAKE3 upper-tree kernel (0 for sha256) */
  float dedup_ms;    /* dict probe + intra-layer dedup + scans + finalize */
  float total_ms;    /* whole enqueue, first to last kernel */
  uint32_t group_log2; /* leaves-per-lane log2 used (BLAKE3) */
  uint32_t reserved;
} ngpu_timing;

/* One chunk of layer file data. 24 bytes.  Chunks lie
 * inside the data buffer and do not overlap (a tar's file extents never do):
 * a descriptor past the buffer, or overlaps adding up to more BLAKE3 leaves
 * than the buffer holds, fail the call with NGPU_EINVAL once its stats are
 * read. */
typedef struct {
  uint64_t offset;      /* byte offset of the chunk in the data buffer */
  uint32_t length;      /* 1 .. chunk_size bytes */
  uint32_t file_index;  /* ordinal of the owning regular file in the tar */
  uint64_t file_offset; /* offset of the chunk inside its file */
} ngpu_chunk;

/* Per-chunk result. 64 bytes. */
typedef struct {
  uint8_t digest[32];   /* BLAKE3-256 or SHA-256 of the raw chunk bytes
                           (RafsV5/V6 ChunkInfo block_id) */
  uint32_t kind;        /* enum ngpu_kind */
  uint32_t index;       /* NEW: sequential chunk index in this layer's blob;
                           INTRA: index of the referenced NEW chunk;
                           DICT: the dict entry's chunk index */
  uint64_t ref;         /* NEW: own chunk id; INTRA: chunk id of the first
                           occurrence; DICT: dict entry id (table order) */
  uint32_t blob_index;  /* real blob index, allocated in first-hit order */
  uint32_t dict_blob;   /* DICT: the entry's inner blob index in the chunk
                           dict (its blob table); otherwise 0 */
  uint64_t uncompressed_offset; /* NEW/INTRA: offset in the layer blob;
                           DICT: the dict chunk's offset in ITS blob (nydus
                           copies the cached chunk, chunk.copy_from) */
} ngpu_result;

/* Summary of one layer. */
typedef struct {
  uint64_t chunks, new_chunks, intra_chunks, dict_chunks;
  uint64_t new_bytes;        /* uncompressed bytes of NEW chunks */
  uint32_t own_blob_index;   /* UINT32_MAX if the layer has no NEW chunk */
  uint32_t blobs;            /* blob-table entries this layer references */
  uint64_t uncompressed_size;/* end of the last NEW chunk (v6: 4K aligned) */
} ngpu_layer_stats;

int ngpu_abi_version(void);

/* Engine lifetime.  Replaces the per-Pack builder process spawn
 * (builder.go:163 exec.CommandContext). */
int ngpu_create(const ngpu_config *cfg, ngpu_engine **out);
void ngpu_destroy(ngpu_engine *eng);
const char *ngpu_last_error(const ngpu_engine *eng);
int ngpu_device_count(void);

/* Pinned host memory owned by the engine (cgo must not hand Go-heap memory
 * to async DMA). */
int ngpu_alloc_pinned(ngpu_engine *eng, uint64_t bytes, void **out);
int ngpu_free_pinned(ngpu_engine *eng, void *ptr);

/* ---- chunk dict handles (PackOption.ChunkDictPath; builder.go:122-124) ----
 * The reference runs one nydus-image process per Pack, each loading its own
 * `--chunk-dict bootstrap=P` ([nydus v2.3.0] HashChunkDict).  Here a dict is
 * an HBM-resident, reference-counted object, immutable per handle
 * (ngpu_dict_extend returns a new one and leaves its base as it was): a Pack
 * captures the dict it is opened with, so packs with different dicts (or none) can be open
 * on one engine at once, and 1000 Packs against one ChunkDictPath share one
 * loaded table.  First table entry wins for duplicate digests; usize == 0
 * matches any chunk size.
 *
 * ngpu_dict_open: load the chunk table (80-B records at the extended
 * superblock's chunk_table_offset, pkg/layout/layout.go:25-27) and the blob
 * table of a RAFS v6 bootstrap on the engine's device.  Rejected with
 * NGPU_EINVAL, as nydus-image rejects an incompatible chunk-dict bootstrap
 * ([nydus v2.3.0] RafsSuperConfig::check_compatibility, VERIFY): a digester
 * flag (RafsSuperFlags HASH_BLAKE3 0x4 / HASH_SHA256 0x8) or chunk_size that
 * differs from the engine's, or an engine with FsVersion 5.  The engine
 * caches the dicts it opened by (path, device, inode, size, mtime): opening an
 * unchanged file again returns the same dict with one more reference. */
typedef struct ngpu_dict ngpu_dict;
int ngpu_dict_open(ngpu_engine *eng, const char *path, ngpu_dict **out);
/* From a chunk table in memory: n 80-B RAFS v6 chunk-info records (table
 * order) and n_blobs 256-B RAFS v6 blob records (inner-index order; may be
 * NULL / 0, the blob count is then max(blob_index) + 1). */
int ngpu_dict_create(ngpu_engine *eng, const void *records, uint64_t n,
                     const void *blob_table, uint32_t n_blobs, ngpu_dict **out);
/* From device-resident arrays (entry order = table order), e.g. a 200M-entry
 * dict built on the GPU.  d_uoff (u64 uncompressed offsets) may be NULL.
 * The build runs on a stream of the library's own and returns when it is
 * done; it does not wait for the caller's streams, so the arrays must be
 * complete when the call is made (synchronise the stream that wrote them). */
int ngpu_dict_create_device(ngpu_engine *eng, const uint8_t *d_digests, const uint32_t *d_usize,
                            const uint32_t *d_blob_index, const uint32_t *d_chunk_index,
                            const uint64_t *d_uoff, uint64_t n, uint32_t n_blobs,
                            ngpu_dict **out);
/* The same with each entry's GLOBAL id (d_gid, device u32; NULL = its
 * position): a rank's digest-prefix share of a dict partitioned across
 * processes (nydus_gpu/dist.py) then answers probes with global entry ids.
 * The rows must be in global table order.  (ABI 4) */
int ngpu_dict_create_device_gid(ngpu_engine *eng, const uint8_t *d_digests,
                                const uint32_t *d_usize, const uint32_t *d_blob_index,
                                const uint32_t *d_chunk_index, const uint64_t *d_uoff,
                                const uint32_t *d_gid, uint64_t n, uint32_t n_blobs,
                                ngpu_dict **out);
/* ---- dict extend: fold a converted layer's records into a dict ----
 * out = base followed by n more 80-B RAFS v6 chunk-info records.  Equal, for every
 * probe, Pack, Check and stats field, to ngpu_dict_create over
 *   records(base) ++ records with blob_index += blobs(base),  blob_table(base) ++ blob_table.
 * First table entry still wins: a digest base already holds keeps base's row.
 * base is not modified and not released; out carries one reference.  flags must be 0.
 *
 * When base is the newest handle on its storage and the storage has room, the
 * records are appended in place (n record writes, n table inserts; no copy,
 * no rebuild: the cost does not depend on base's size) and out shares base's
 * HBM; otherwise out gets a storage half as large again, base's records are
 * copied device to device and the table is built over all of them.  A dict from
 * ngpu_dict_open / ngpu_dict_create* is allocated exactly, so its first extend
 * copies.  Handles of one storage free it when the last of them is released.
 * Safe against probes of base (and of any older handle) running on other
 * streams and threads meanwhile; two threads extending one base at once get
 * one in-place result and one copy.  The device work runs on a stream of the
 * library's own and is complete when the call returns.
 *
 * Rejected before any GPU work: base == NULL, flags != 0 or n && !records
 * (NGPU_EINVAL); entries(base) + n >= 0xFFFFFFFF or more than 2^20 blobs (as
 * ngpu_dict_create); a record whose blob_index >= n_blobs when a table is given
 * (NGPU_EFORMAT); a node dict (NGPU_EINVAL: ngpu_node_dict_extend).  Blob table:
 * out has one iff base has one and the call passes one; when neither does, out
 * has only a blob count; exactly one side with a table is NGPU_EINVAL (nothing
 * is dropped silently).  A base of 0 blobs goes with either, and so does a call
 * with n == 0 and no table, which returns a handle equal to base.  out keeps
 * compressed placements (what a Pack's DICT records copy) iff base did or base
 * was empty.  On failure *out is NULL and base is untouched. */
int ngpu_dict_extend(ngpu_engine *eng, ngpu_dict *base, const void *records, uint64_t n,
                     const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out);
/* The same from a RAFS v6 bootstrap file (its chunk table and blob table), with
 * ngpu_dict_open's compatibility checks (digester flag, chunk size, FsVersion 6). */
int ngpu_dict_extend_bootstrap(ngpu_engine *eng, ngpu_dict *base, const char *path,
                               uint32_t flags, ngpu_dict **out);
/* ---- dict extend from device arrays (additive in ABI 7) ----
 * ngpu_dict_extend for rows that lie in HBM as ngpu_dict_create_device's arrays
 * (d_uoff and d_chunk_index may be NULL; the arrays must be complete when the
 * call is made).  out answers every probe, Pack, Check, stats field and export as
 * ngpu_dict_extend over the same rows given as 80-B records without a blob table:
 * blob_index += blobs(base), entry ids entries(base) + position, in place or on a
 * larger storage exactly as ngpu_dict_extend decides.  Nothing is staged: one
 * kernel writes the records behind base's, the table insert (or build) follows.
 * n_blobs is the caller's word for the new rows' blob count, as in
 * ngpu_dict_create_device; blobs(out) = blobs(base) + n_blobs, at most 2^20.
 * The call carries no blob table and no compressed placements, so a base that
 * holds a blob table is NGPU_EINVAL (ngpu_dict_extend's rule: exactly one side
 * with a table; a base of 0 blobs is fine), and so is a base that keeps
 * placements when n > 0: nothing is dropped silently.  n == 0 returns a handle
 * equal to base.  Also NGPU_EINVAL, all with *out = NULL: base == NULL,
 * flags != 0, n without d_digests / d_usize / d_blob_index, d_digests not
 * 16-byte aligned, a node dict.  The device work runs on a stream of the
 * library's own, outside the engine lock, and is complete on return; one fold
 * or extend_device runs at a time per engine. */
int ngpu_dict_extend_device(ngpu_engine *eng, ngpu_dict *base, const uint8_t *d_digests,
                            const uint32_t *d_usize, const uint32_t *d_blob_index,
                            const uint32_t *d_chunk_index, const uint64_t *d_uoff, uint64_t n,
                            uint32_t n_blobs, uint32_t flags, ngpu_dict **out);
/* ---- dict fold: grow a dict from a dedup call's results (additive in ABI 7) ----
 * out = base followed by one record per chunk of d_results[0, n) whose kind ==
 * NGPU_NEW, in chunk order (layers are contiguous in chunk order: layer order,
 * then stream order inside a layer).  d_results / d_chunks are the device tables
 * of an ngpu_process*_device / ngpu_dedup*_device call, d_layer_first its
 * n_layers + 1 device u64 layer cuts (NULL or n_layers <= 1: one layer of n
 * chunks).  Equal, for every probe, Pack, Check, stats field and export, to
 * ngpu_dict_extend over the host rows built from each NEW chunk c:
 *   block_id            = d_results[c].digest
 *   uncompressed_size   = d_chunks[c].length
 *   blob_index          = r(l): the number of layers before c's layer l that hold
 *                         at least one NEW chunk (every such layer is one new
 *                         blob; after the shift the record's blob is
 *                         blobs(base) + r(l))
 *   index               = d_results[c].index
 *   uncompressed_offset = d_results[c].uncompressed_offset
 *   compressed_offset / compressed_size / flags = placements[position among the
 *                         new records] (host rows), or csize = usize, offset 0,
 *                         flags 0 when the dict keeps none
 * INTRA and DICT chunks add nothing.  First entry still wins; base is untouched
 * and not released; handles older than out stay blind to an in-place append;
 * share or fork as ngpu_dict_extend decides.  flags must be 0.
 *
 * The NEW chunks k and the layers with one, b, are counted on the device (one
 * keep bit per chunk, a scan, a pass over the layers) and come back in one small
 * copy, the call's only mid-way wait; everything below is then checked before a
 * byte of any storage is written and before a record slot is reserved, so a
 * refused call leaves base and its storage as they were.  Refused with
 * NGPU_EINVAL and *out = NULL:
 *   a kind other than NEW / INTRA / DICT anywhere in [0, n) (DIGESTED, UNHASHED,
 *   garbage): the message names the first such chunk;
 *   a NEW chunk with length 0 or > chunk_size;
 *   layer cuts with first[0] != 0, first[n_layers] != n or a decreasing entry;
 *   d_results not 16-byte aligned, d_chunks / d_layer_first not 8-byte aligned,
 *   n without d_results / d_chunks;
 *   placements with n_placements != k; k > 0 and base keeps placements but none
 *   are given; base has records and keeps none but some are given (an empty
 *   base goes with either);
 *   the blob table: ngpu_dict_extend's rule, and n_blobs == b when one is
 *   passed (n_blobs without blob_table is refused);
 *   ngpu_dict_extend's size limits; a node dict; flags != 0.
 * k == 0 returns a handle equal to base.  The device work runs on a stream of the
 * library's own, outside the engine lock, and is complete on return; it does not
 * wait for the caller's streams, so the stream that wrote the results must have
 * been synchronised (as for ngpu_dict_create_device).  An in-place fold
 * allocates and frees no device memory. */
typedef struct {
  uint64_t compressed_offset;
  uint32_t compressed_size;
  uint32_t flags; /* RAFS v6 chunk flags (bit 0: compressed) */
} ngpu_dict_place;
int ngpu_dict_fold(ngpu_engine *eng, ngpu_dict *base, const ngpu_result *d_results,
                   const ngpu_chunk *d_chunks, uint64_t n, const uint64_t *d_layer_first,
                   uint64_t n_layers, const ngpu_dict_place *placements, uint64_t n_placements,
                   const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out);
/* ---- dict retire: drop the records of deleted blobs from a dict ----
 * out = base without the records of the listed inner blobs (blobs[0, n), any
 * order, duplicates allowed).  Equal, for every probe, Pack, Check, stats field
 * and export, to ngpu_dict_create over a filtered copy of base:
 *   the records of base, in table order, whose blob_index is not listed, each
 *   with blob_index replaced by its rank among the kept blobs;
 *   the blob table rows of the kept blobs, in order.  A base with only a blob
 *   count gives out only the new count: blobs(base) - distinct listed blobs.
 * Entry ids are positions among the survivors.  First table entry still wins:
 * when the winning row of a digest leaves, the next surviving row with that
 * digest wins.  out keeps compressed placements iff base did.  Only the handle's
 * own entries(base) records count: rows a later in-place extend appended to the
 * same storage are not seen.  base is not modified and not released; out carries
 * one reference.  flags must be 0.
 *
 * out always sits on a storage of its own (nothing a live handle can see is
 * written, so probes of base may run meanwhile on other streams and threads),
 * sized like the copy of an extend that adds nothing: s + s / 2 record slots
 * for s survivors and the table ngpu_dict_create gives for that many, so that
 * the next extends of out, up to s / 2 records in all, append in place.  n == 0
 * is a compacting copy equal to base (the way to drop the id ranges a failed
 * extend or an abandoned tip left dead on a storage).  Retiring every blob gives
 * a valid dict of 0 entries and 0 blobs: it dedups nothing and can be extended.
 * The device work (keep bits, their scan, the compaction, the table build) runs
 * on a stream of the library's own, outside the engine lock, and is complete
 * when the call returns.
 *
 * Rejected before any GPU work, with *out = NULL: base == NULL, flags != 0 or
 * n && !blobs (NGPU_EINVAL); an index >= blobs(base) (NGPU_EINVAL); a node dict
 * (NGPU_EINVAL: ngpu_node_dict_retire).  On failure base is untouched. */
int ngpu_dict_retire(ngpu_engine *eng, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                     uint32_t flags, ngpu_dict **out);
/* ---- dict distill: one row per digest, kept by how many rows hold it ----
 * (additive in ABI 7).  A probe stops at the first row of a digest, so every
 * later row with the same 32 digest bytes can never answer: it only costs HBM, a
 * placement row, and time in every save and open.  refs(d) is the number of rows
 * of base[0, entries(base)) whose 32 digest bytes are d (uncompressed_size takes
 * no part: this is the table's own view); the winner of d is its first row.
 *
 * out equals, for every probe, Pack, Check, stats field, export and save,
 * ngpu_dict_create over:
 *   the winners of base, in table order, whose refs >= max(min_refs, 1), each
 *   unchanged but for its blob index;
 *   the blob rows as the flags say (below).
 * Entry ids are positions among the survivors.  min_refs <= 1 is the pure
 * clean-up: every digest answers as in base (same blob id, chunk index,
 * uncompressed offset, size and placement); only the entry ids and the inner blob
 * indices are renumbered.  A larger min_refs keeps the chunks that recur (a row
 * per layer that referenced the chunk: what nydus's `chunkdict generate` selects
 * by) and lets go of the rest; above every count it gives a valid dict of 0
 * entries and 0 blobs, which dedups nothing and can be extended.  out keeps
 * compressed placements iff base did.
 *
 * Blobs.  By default a blob with no surviving row leaves, one that never had a row
 * included, and the rest are re-ranked in order, exactly as ngpu_dict_retire does;
 * a base with only a blob count gives out only the new count.
 * NGPU_DICT_DISTILL_KEEP_BLOBS: blob indices and the blob table stay as they are.
 * NGPU_DICT_DISTILL_MERGE_BLOB_IDS: every blob whose 256-B row starts with the
 * same 64 id bytes as an earlier blob's is mapped to the earliest one, whose row
 * is the one kept; it is live if any of the merged blobs has a survivor.  Refs
 * still count rows.  It needs a blob table.  Rows whose blob is >= blobs(base)
 * (ngpu_dict_create_device takes the caller's word) are kept as they are and make
 * no blob live, as in a retire.
 *
 * Only the handle's own entries(base) rows count: rows a later in-place extend
 * appended to the same storage are not seen.  base is only read: probes, Packs and
 * in-place extends of base may run meanwhile.  out always sits on a storage of its
 * own with ngpu_dict_retire's room (s + s / 2 record slots for s survivors), so
 * the next extends of up to s / 2 records append in place.  The device work (the
 * counts, the keep bits, their scan, the compaction, the table build) runs on a
 * stream of the library's own, outside the engine lock, and is complete when the
 * call returns.  out == NULL only counts: info is filled and no storage is
 * allocated.  info (may be NULL) is filled on every successful call and zeroed on
 * every failure.
 *
 * What a distill gives up: after a retire, when the winning row of a digest
 * leaves, the next surviving row with that digest wins.  A distilled dict has no
 * next row: retiring the blob of a digest's one row forgets the digest, even if
 * base held it in other blobs too.  Distill trades that fallback for the space.
 *
 * Rejected before any GPU work, with *out = NULL (NGPU_EINVAL): base or eng NULL,
 * flag bits other than the two, both flags together (with KEEP_BLOBS nothing is
 * merged), MERGE_BLOB_IDS on a dict with records and no blob table, a node dict
 * (ngpu_node_dict_distill). */
#define NGPU_DICT_DISTILL_KEEP_BLOBS     0x1u /* leave blob indices and the blob table as they are */
#define NGPU_DICT_DISTILL_MERGE_BLOB_IDS 0x2u /* blob rows with the same 64-byte blob id become the first of them */
typedef struct {
  uint64_t entries_in;    /* entries(base) */
  uint64_t distinct;      /* digests base holds: rows that win their digest */
  uint64_t shadowed;      /* entries_in - distinct */
  uint64_t below_min;     /* distinct digests held by fewer than min_refs rows */
  uint64_t entries_out;   /* distinct - below_min */
  uint32_t blobs_in, blobs_out;
  uint32_t max_refs;      /* the most rows any one digest has (0 for an empty dict) */
  uint32_t reserved;
  uint64_t refs_hist[32]; /* [b]: distinct digests with 2^b <= refs < 2^(b+1) */
} ngpu_dict_distill_info; /* 312 bytes */
int ngpu_dict_distill(ngpu_engine *eng, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                      ngpu_dict **out /* NULL: count only */, ngpu_dict_distill_info *info /* may be NULL */);
/* The handle's rows back out of HBM: entries(d) 80-B RAFS v6 chunk-info records in
 * table order and its 256-B blob records, such that ngpu_dict_create over them
 * answers as d does.  block_id, blob_index, uncompressed_size, uncompressed_offset
 * and index come from the HBM rows; compressed_offset, compressed_size and flags
 * from the placement rows (a dict without them: compressed_size =
 * uncompressed_size, offset 0, flags 0, as ngpu_dict_load documents); file_offset
 * and the reserved word are 0.  *n_records = entries(d) and *n_blobs = blobs(d) are
 * always set.  records == NULL && cap == 0 only counts; cap < entries(d) is
 * NGPU_EINVAL and nothing is written.  The blob table is written when blob_table
 * is given and the handle has one (ngpu_dict_info.has_blob_table; blob_cap rows
 * of room, too few: NGPU_EINVAL, nothing written).  Plain dicts and replicated
 * node dicts (part 0's rows, the node handle's placements); a partitioned node
 * dict returns NGPU_EUNSUPP here: ngpu_node_dict_export takes both node modes. */
int ngpu_dict_export(ngpu_engine *eng, const ngpu_dict *d, void *records, uint64_t cap,
                     uint64_t *n_records, void *blob_table, uint32_t blob_cap, uint32_t *n_blobs);
typedef struct {
  uint64_t entries, blobs;
  uint64_t record_capacity, table_capacity; /* of the storage it sits on (node dict: part 0) */
  uint32_t shares_base_storage;             /* 1: made by an in-place extend */
  uint32_t has_blob_table;                  /* 1: it holds 256-B blob records (a reserved,
                                               zero word until dict retire; still ABI 7) */
  uint32_t reserved[2];
} ngpu_dict_info;
int ngpu_dict_info_get(const ngpu_dict *d, ngpu_dict_info *out);
void ngpu_dict_retain(ngpu_dict *d);
void ngpu_dict_release(ngpu_dict *d);
uint64_t ngpu_dict_entries(const ngpu_dict *d);
/* The engine's default dict, used by the calls without a dict argument
 * (ngpu_process*, ngpu_pack_open*, ngpu_dict_probe_device) and captured by a
 * pack when it opens.  NULL = no dict.  Takes a reference. */
int ngpu_set_dict(ngpu_engine *eng, ngpu_dict *d);

/* Legacy default-dict loaders (each = create + ngpu_set_dict + release).
 * Replacing the default never changes the dict of a pack already open.
 * ngpu_dict_load: n entries in chunk-table order; blob_index: inner blob index
 * per entry; chunk_index: the entry's RAFS chunk index (copied into DICT
 * results); compressed placement unknown (csize = usize, offsets 0). */
int ngpu_dict_load(ngpu_engine *eng, const uint8_t *digests /* n x 32 */,
                   const uint32_t *usize, const uint32_t *blob_index,
                   const uint32_t *chunk_index, uint64_t n);
int ngpu_dict_load_bootstrap(ngpu_engine *eng, const char *path);
int ngpu_dict_clear(ngpu_engine *eng);
uint64_t ngpu_dict_size(const ngpu_engine *eng);

/* ---- tar front end (host) ------------------------------------------------ */
/* Enumerate the chunks of a tar-rafs layer.  Writes at
 * most cap chunks; *n_chunks receives the full count (call again with a
 * larger array if it exceeds cap).  *n_files: regular files seen. */
int ngpu_tar_chunks(const void *tar, uint64_t len, uint32_t chunk_size,
                    ngpu_chunk *out, uint64_t cap, uint64_t *n_chunks,
                    uint64_t *n_files);

/* ---- digest + dedup ------------------------------------------------------- */
/* Host buffers in, host results out (synchronous).  `data` is the layer's
 * bytes (e.g. the uncompressed tar), `chunks` index into it.  Data moves to
 * HBM through the engine's pinned staging slots with hipMemcpyAsync. */
int ngpu_process(ngpu_engine *eng, const void *data, uint64_t len,
                 const ngpu_chunk *chunks, uint64_t n, ngpu_result *out,
                 ngpu_layer_stats *stats);

/* Device-resident variant: data, chunks and out are device pointers; work is
 * enqueued on `stream` (a hipStream_t; NULL = the null/default stream, as in
 * HIP itself) and the call returns without synchronising, so it is stream-
 * ordered after whatever the caller enqueued on the same stream to produce
 * d_data / d_chunks.  stats may be NULL; if not NULL the call synchronises
 * the stream to fill it.  The same holds for every *_device entry point
 * below except ngpu_dict_load_device (synchronous: its inputs must be
 * complete when it is called). */
int ngpu_process_device(ngpu_engine *eng, const void *d_data, uint64_t len,
                        const ngpu_chunk *d_chunks, uint64_t n,
                        ngpu_result *d_out, void *stream,
                        ngpu_layer_stats *stats);

/* ---- split stages (device pointers, async on `stream`) -------------------
 * For callers that route dict probes themselves, e.g. a chunk dict
 * partitioned across GPUs by digest prefix:
 *   ngpu_digest_device     -> digests only (d_out[i].digest);
 *   ngpu_dict_probe_device -> look digests up in THIS engine's dict;
 *   ngpu_dedup_device      -> dedup decisions from digests + given dict hits.
 * ngpu_process_device == digest + dedup against the engine's own dict. */
typedef struct {
  uint32_t entry;  /* dict entry id (chunk-table order) or 0xFFFFFFFF: miss */
  uint32_t index;  /* the entry's RAFS chunk index */
  uint32_t blob;   /* the entry's inner blob index */
  uint32_t usize;  /* the entry's uncompressed size (0 = any) */
  uint64_t uncompressed_offset; /* the entry's offset in its blob */
} ngpu_dict_hit;   /* 24 bytes */

int ngpu_digest_device(ngpu_engine *eng, const void *d_data, uint64_t len,
                       const ngpu_chunk *d_chunks, uint64_t n,
                       ngpu_result *d_out, void *stream);
/* d_digests: n digests at byte stride `stride` (32 for packed, 64 to read
 * ngpu_result.digest in place).  No size rule is applied here: the hit
 * carries usize and the requester's dedup applies it. */
int ngpu_dict_probe_device(ngpu_engine *eng, const uint8_t *d_digests,
                           uint64_t stride, uint64_t n,
                           ngpu_dict_hit *d_hits, void *stream);
/* d_hits: per-chunk dict hits (NULL: probe this engine's dict).
 * n_dict_blobs: number of inner blobs of the (global) chunk dict; 0 = use
 * this engine's dict.  stats as in ngpu_process_device. */
int ngpu_dedup_device(ngpu_engine *eng, const ngpu_chunk *d_chunks, uint64_t n,
                      ngpu_result *d_out, const ngpu_dict_hit *d_hits,
                      uint32_t n_dict_blobs, void *stream,
                      ngpu_layer_stats *stats);
/* Many layers per call (e.g. 1000 small layers against one chunk dict):
 * layer l owns chunks [d_layer_first[l], d_layer_first[l+1]) (device u64
 * array of n_layers+1, d_layer_first[n_layers] == n).  Each layer is deduped
 * exactly as if it were packed alone (its own layered dict, NEW indices,
 * offsets and blob order); the chunk dict is shared.  d_stats: device
 * ngpu_layer_stats[n_layers] (written asynchronously), or NULL. */
int ngpu_dedup_layers_device(ngpu_engine *eng, const ngpu_chunk *d_chunks, uint64_t n,
                             ngpu_result *d_out, const ngpu_dict_hit *d_hits,
                             uint32_t n_dict_blobs, const uint64_t *d_layer_first,
                             uint64_t n_layers, ngpu_layer_stats *d_stats, void *stream);
int ngpu_process_layers_device(ngpu_engine *eng, const void *d_data, uint64_t len,
                               const ngpu_chunk *d_chunks, uint64_t n, ngpu_result *d_out,
                               const uint64_t *d_layer_first, uint64_t n_layers,
                               ngpu_layer_stats *d_stats, void *stream);
/* Build the default dict from device-resident arrays (entry order = table
 * order); = ngpu_dict_create_device + ngpu_set_dict. */
int ngpu_dict_load_device(ngpu_engine *eng, const uint8_t *d_digests,
                          const uint32_t *d_usize, const uint32_t *d_blob_index,
                          const uint32_t *d_chunk_index, uint64_t n,
                          uint32_t n_blobs);

/* The same against an explicit dict (NULL = no chunk dict) instead of the
 * engine's default.  ngpu_process_dict_device: d_layer_first NULL = one layer
 * of n chunks (n_layers ignored); d_stats: device ngpu_layer_stats[n_layers]
 * or NULL; stats: host, as in ngpu_process_device (synchronises), one-layer
 * calls only. */
int ngpu_dict_probe(const ngpu_dict *dict, const uint8_t *d_digests, uint64_t stride,
                    uint64_t n, ngpu_dict_hit *d_hits, void *stream);

/* Digest-prefix routing for a dict partitioned over `world` owners (<= 64;
 * owner(d) = ((d[0] << 8 | d[1]) * world) >> 16), device pointers, async on
 * `stream` (ABI 4).  Each of the n digests (byte stride `stride`, 16-B
 * aligned) goes to its owner's segment of d_out (32 B per row) with its row id
 * in d_rows.  d_counts: 128 device u32, written by the call: [0, world) =
 * rows per owner.  seg_cap == 0: owners back to back in owner order (owner o
 * at the sum of the counts before it), d_out / d_rows hold n rows.  seg_cap >
 * 0 (equal splits): row k of owner o goes to slot [k / seg_cap][o][k %
 * seg_cap] of rounds x world x seg_cap slots; the call zeroes d_out and sets
 * every d_rows slot to 0xFFFFFFFF first (padding), and rounds * seg_cap must
 * cover n.  Order inside a segment is unspecified: hits return by row id. */
int ngpu_route_digests(const uint8_t *d_digests, uint64_t stride, uint64_t n, uint32_t world,
                       uint64_t seg_cap, uint32_t rounds, uint8_t *d_out, uint32_t *d_rows,
                       uint32_t *d_counts, void *stream);
/* d_hits[d_rows[i]] = d_routed[i] for the m routed rows (rows of 0xFFFFFFFF,
 * padding, are skipped): an owner's hits back in the requester's row order. */
int ngpu_route_hits(const ngpu_dict_hit *d_routed, const uint32_t *d_rows, uint64_t m,
                    ngpu_dict_hit *d_hits, void *stream);
int ngpu_process_dict(ngpu_engine *eng, ngpu_dict *dict, const void *data, uint64_t len,
                      const ngpu_chunk *chunks, uint64_t n, ngpu_result *out,
                      ngpu_layer_stats *stats);
int ngpu_process_dict_device(ngpu_engine *eng, ngpu_dict *dict, const void *d_data,
                             uint64_t len, const ngpu_chunk *d_chunks, uint64_t n,
                             ngpu_result *d_out, const uint64_t *d_layer_first,
                             uint64_t n_layers, ngpu_layer_stats *d_stats, void *stream,
                             ngpu_layer_stats *stats);

/* Whole tar layer in host memory -> chunk list + results (tar parse on the
 * host, digest/dedup on the GPU).  *chunks_out / *results_out are allocated
 * with malloc and must be released with ngpu_free_host. */
int ngpu_pack_tar(ngpu_engine *eng, const void *tar, uint64_t len,
                  ngpu_chunk **chunks_out, ngpu_result **results_out,
                  uint64_t *n_out, ngpu_layer_stats *stats);
void ngpu_free_host(void *p);

/* Batched Pack closes so far (NGPU_FLAG_NO_BATCH): out[0] launch sets,
 * out[1] packs closed in them, out[2] the most packs in one. */
int ngpu_batch_stats(ngpu_engine *eng, uint64_t out[3]);
/* Stage timings of the last ngpu_process / ngpu_process_device call on this
 * engine (synchronises on the recorded events).  NGPU_EINVAL unless the
 * engine was created with NGPU_FLAG_TIMING. */
int ngpu_last_timing(ngpu_engine *eng, ngpu_timing *out);
/* The same for the call `back` calls before the last one (0 = the last).
 * The engine keeps the events of its last 64 calls, so a caller can time a
 * run of back-to-back calls without synchronising between them. */
int ngpu_timing_at(ngpu_engine *eng, uint32_t back, ngpu_timing *out);

/* ---- streaming Pack (converter.Pack, pkg/converter/convert_unix.go:325) ----
 * The reference returns an io.WriteCloser fed with the uncompressed layer tar
 * (packFromTar :443-539 pipes it to nydus-image through a FIFO).  Here:
 * open -> write (copying) or reserve/commit (zero-copy into engine-pinned
 * staging) in any split -> close.  Full staging slots are copied to HBM and
 * digested while the caller keeps writing; dedup runs at close in stream
 * order.  close (success or not) and abort release the pack; *chunks_out /
 * *results_out are malloc'd (ngpu_free_host).  A malformed or truncated tar
 * fails with NGPU_ETAR / NGPU_EUNSUPP at write/commit or close.
 * A pack dedups against the dict it was opened with: ngpu_pack_open* take the
 * engine's default dict at open time, ngpu_pack_open_dict an explicit one
 * (NULL = none; its digester and chunk size must be the engine's). */
typedef struct ngpu_pack ngpu_pack;
int ngpu_pack_open(ngpu_engine *eng, ngpu_pack **out);
int ngpu_pack_open_dict(ngpu_engine *eng, ngpu_dict *dict, uint32_t flags, ngpu_pack **out);
/* Cancellation (ctx.Done() / PackOption.Timeout): `flag` is caller-owned
 * memory that must outlive the pack; once another thread stores a non-zero
 * value there, the pack's next write / commit / reserve, or the running
 * close / finish at its next slot, blob window or compression batch, fails
 * with NGPU_ECANCELED (the reference kills the builder process,
 * builder.go:153-174, convert_unix.go:530-535).  close / finish release the
 * pack on every outcome; after a failed write / commit / reserve the pack
 * stays open until the caller aborts it (ngpu_pack_abort).  NULL removes the
 * flag. */
int ngpu_pack_set_cancel(ngpu_pack *p, const volatile int32_t *flag);
int ngpu_pack_write(ngpu_pack *p, const void *buf, uint64_t len);
int ngpu_pack_reserve(ngpu_pack *p, void **ptr, uint64_t *avail);
int ngpu_pack_commit(ngpu_pack *p, uint64_t n);
int ngpu_pack_close(ngpu_pack *p, ngpu_chunk **chunks_out, ngpu_result **results_out,
                    uint64_t *n_out, ngpu_layer_stats *stats);
/* Ends a pack without output: its staging, HBM and emitter thread are
 * released.  A binding calls it on every path that will never reach close --
 * a failed write, a source read error, ctx.Done() with no Close to follow
 * (convert_unix.go:885-907 skips tw.Close() on those paths).  Not concurrently
 * with another call on the same pack. */
void ngpu_pack_abort(ngpu_pack *p);
/* The engine a pack runs on (borrowed; e.g. to see where ngpu_node_pack_open
 * placed it: compare with ngpu_node_engine).  (ABI 7) */
ngpu_engine *ngpu_pack_engine(const ngpu_pack *p);

/* What an engine holds right now (ABI 7): a leak check for the bindings'
 * error paths (every aborted or finished pack gives all of it back). */
typedef struct {
  uint64_t open_packs;          /* packs opened and not yet ended */
  uint64_t staging_pool_bufs;   /* pinned staging slots kept for the next packs */
  uint64_t staging_pool_bytes;  /* their pinned bytes */
  uint64_t pack_pool;           /* per-pack stream + buffer sets kept */
  uint64_t land_pool;           /* early-emission landing buffers kept */
  uint64_t batch_waitable;      /* open packs a batch leader would still wait for */
  uint64_t check_windows;       /* staging windows Check has sent to the GPU so far (a
                                   reserved word until Check; still ABI 7) */
  uint64_t reserved[1];
} ngpu_engine_counters;
int ngpu_engine_counters_get(ngpu_engine *eng, ngpu_engine_counters *out);

/* ---- multi-GPU node ------------------------------------
 * One process drives the GPUs of a node: one engine per listed device (a
 * device may be listed twice, e.g. to rehearse a 2-GPU node on one GPU).
 * Layers are independent units (north star: "the chunk stream is sharded by
 * layer"): ngpu_node_pack_open places each streaming Pack on the engine with
 * the fewest open packs (ties round robin) -- containerd's per-layer
 * goroutines (convert_unix.go:467-538) then spread over every GPU and every
 * GPU's own PCIe link -- and ngpu_node_process_device runs device-resident
 * layers on a chosen engine.  A node chunk dict is either partitioned by
 * digest prefix -- entry with digest d lives on device
 * ((d[0] << 8 | d[1]) * n) >> 16, keeping table order, so "first entry wins"
 * holds per digest -- or replicated on every device.  Probing a partitioned
 * dict is the node's exchange step: the requester's digests go to every
 * owner, each owner probes the entries it owns and the hits come back with
 * GLOBAL entry ids, ordered by cross-device events -- the in-process form of
 * the north star's digest-prefix all-to-all (nydus_gpu/dist.py keeps the
 * one-process-per-GPU RCCL form).  Default exchange (ABI 7, "copy"): every
 * digest to every owner and every owner's n hits back by hipMemcpyPeerAsync
 * (DMA engines; W x n x 56 bytes per call), merged by owner on the
 * requester.  NGPU_NODE_EXCHANGE_ROUTED in `mode` (opt-in, the ABI 4-6
 * default) runs the routed exchange instead when every pair of listed devices
 * has peer access: the requester buckets its digests by owner in its own HBM;
 * each owner's probe kernel reads only its own rows (peer loads over xGMI)
 * and writes each hit into the requester's hit array at the row's id (peer
 * stores), so a call moves n x (32 + 4) bytes out and n x 24 back in total.
 * Peer access between the listed devices is enabled at creation.
 * UNVERIFIED ON DISTINCT GPUs: every test so far lists one GPU several times
 * (the copies and peer stores then stay inside one HBM); the routed
 * exchange's peer stores, the copy exchange and the RCCL node step first
 * meet separate GPUs in the driver's multi-GPU bench, whose `node_cabi` entry
 * runs all three against a replicated dict, prints them in its
 * `multi_gpu_checks` summary and fails the run if any disagrees.  Until that
 * has passed, a caller that needs certainty uses NGPU_NODE_DICT_REPLICATE (no
 * exchange), as the converter mirrors do for ChunkDictPath. */
typedef struct ngpu_node ngpu_node;
int ngpu_node_create(const int32_t *devices, uint32_t n, const ngpu_config *cfg, ngpu_node **out);
void ngpu_node_destroy(ngpu_node *node);
uint32_t ngpu_node_size(const ngpu_node *node);
/* The node's engine i (borrowed: valid until ngpu_node_destroy). */
ngpu_engine *ngpu_node_engine(ngpu_node *node, uint32_t i);
#define NGPU_NODE_DICT_PARTITION 0u /* shard by digest prefix (default) */
#define NGPU_NODE_DICT_REPLICATE 1u /* a full copy on every device */
#define NGPU_NODE_EXCHANGE_COPY 0x100u   /* | PARTITION: broadcast + DMA exchange (default) */
#define NGPU_NODE_EXCHANGE_ROUTED 0x200u /* | PARTITION: peer-kernel exchange (opt-in) */
/* Node chunk dicts, usable by any engine of the node (ngpu_pack_open_dict,
 * ngpu_process_dict*, ngpu_node_*); checks as ngpu_dict_open.
 * ngpu_node_dict_open caches what it opened, as ngpu_dict_open does per
 * engine: opening an unchanged file (path, device, inode, size, mtime) with
 * the same mode again returns the same dict with one more reference, so 1000
 * Packs naming one ChunkDictPath load it once per node. */
int ngpu_node_dict_open(ngpu_node *node, const char *path, uint32_t mode, ngpu_dict **out);
/* ngpu_dict_extend for node dicts: a partitioned dict gives each part the
 * records it owns (global ids entries(base) + position), a replicated one gives
 * every replica all of them; the exchange mode is base's.  Each part appends
 * in place or copies by its own fill.  A plain dict here is NGPU_EINVAL. */
int ngpu_node_dict_extend(ngpu_node *node, ngpu_dict *base, const void *records, uint64_t n,
                          const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out);
/* ---- node dict fold: grow a node dict from a step's results (additive in ABI 7) ----
 * ngpu_dict_fold for node dicts: part i is the result table of a dedup /
 * process / step call on node device i (ngpu_node_process_step,
 * ngpu_node_process_device), with its descriptors and layer cuts as
 * ngpu_dict_fold takes them; a part with n == 0 takes part with nothing.  out
 * answers every probe, Pack, Check, stats field and (replicated dicts) export
 * exactly as ngpu_node_dict_extend over the concatenated host rows: part 0's fold
 * rows, then part 1's, ..., each part's rows as ngpu_dict_fold defines them (one
 * per kind == NGPU_NEW chunk, in chunk order), with blob ranks that run on across
 * the parts: the blob rank of layer l of part i is the number of layers with a
 * NEW chunk in the parts before i plus those before l in part i.  placements
 * and blob_table rows are given in that same global order (k = all parts' NEW
 * chunks, b = all parts' layers with one).
 *
 * First entry wins: base over new rows, and a digest NEW in two parts keeps the
 * lower part's row.  Handles older than out stay blind to an in-place append;
 * each part appends in place or copies by its own fill; the exchange mode and
 * replicated / partitioned are base's.  k == 0 over all parts returns a handle
 * equal to base.
 *
 * Every refusal of ngpu_dict_fold applies to each part (the message names the
 * part and the chunk or layer), its placement and blob-table rules to k and b.
 * Also NGPU_EINVAL: n_parts != ngpu_node_size(node); flags != 0; a plain dict or
 * a dict of another node (ngpu_dict_fold keeps refusing node dicts).  All
 * refusals are decided after the counts of all parts are back -- one small copy
 * per part, all parts enqueued before the first wait, the call's only mid-way
 * one -- and before any part's record slot is reserved or a storage byte is
 * written: a refused call leaves every part as it was.  A failure after that
 * point behaves as in ngpu_node_dict_extend: *out is NULL, base stays usable,
 * id ranges may be left dead.
 *
 * The rows never pass through the host: each part's rows are written into a
 * staging area on its own device with their final global ids and blobs, a
 * partitioned dict splits them by owner there (a stable split: an owner's rows
 * stay in global table order), and every part then copies the rows it keeps
 * with DMA copies (hipMemcpyPeerAsync between devices), no peer stores from
 * kernels.  The device work runs on each engine's own fold stream, outside the
 * engine locks, and is complete on return; it does not wait for the caller's
 * streams, so the streams that wrote the results must have been synchronised.
 * Once warm, an in-place fold allocates and frees no device memory.
 * UNVERIFIED ON DISTINCT GPUs, as the node exchange above: every test so far
 * lists one GPU several times, so the peer copies stay inside one HBM. */
typedef struct {
  const ngpu_result *d_results;  /* on node device i: a dedup / process / step call's result table */
  const ngpu_chunk *d_chunks;    /* its n descriptors */
  uint64_t n;
  const uint64_t *d_layer_first; /* n_layers + 1 cuts on that device; NULL or n_layers <= 1: one layer */
  uint64_t n_layers;
} ngpu_node_fold_part;           /* 40 bytes */
int ngpu_node_dict_fold(ngpu_node *node, ngpu_dict *base, const ngpu_node_fold_part *parts,
                        uint32_t n_parts, const ngpu_dict_place *placements, uint64_t n_placements,
                        const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out);
/* ngpu_dict_retire for node dicts.  A replicated dict retires every replica
 * with the same result (global id = position) and the node handle's placement
 * rows follow.  A partitioned dict returns NGPU_EUNSUPP from this call, as it
 * always has: ngpu_node_dict_retire_parts retires both modes.  A plain dict here
 * is NGPU_EINVAL.  *out is NULL on every failure and base stays usable. */
int ngpu_node_dict_retire(ngpu_node *node, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                          uint32_t flags, ngpu_dict **out);
/* ngpu_dict_retire for node dicts of both modes (additive in ABI 7).  A replicated
 * dict goes the way of ngpu_node_dict_retire.  For a partitioned dict the contract
 * is ngpu_dict_retire's, stated on the whole dict: out answers every probe, Pack,
 * ngpu_node_process_device / _step and export as ngpu_node_dict_create does, in
 * base's mode and exchange, over base's records without those of the listed blobs.
 * Records stay in global table order, kept blobs are re-ranked, the kept blob
 * table rows and the placement rows are kept iff base had them, entry ids (the
 * global ids the parts' hits carry) are positions among ALL parts' survivors, and
 * the first entry still wins.  Only the handle's own entries(base) count: rows a
 * later in-place extend or fold appended to the parts' storages are not seen.
 * base is only read: probes of it may run meanwhile.
 *
 * Every part of out sits on a storage of its own with ngpu_dict_retire's room for
 * its own survivors (s + s / 2 record slots), the node handle on placement rows
 * for all of them, so later extends and folds append in place.  n == 0 is a
 * compacting copy; retiring every blob gives a valid dict of 0 entries.  The
 * device work runs on streams of the library's own, one per part, which exchange
 * one keep bit per entry of base between the parts (W x entries / 8 bytes into
 * every part); all of them are synchronised when the call returns, on every path.
 *
 * Rejected before any GPU work, with *out = NULL: a NULL argument, flags != 0,
 * n && !blobs, an index >= blobs(base), a plain dict, a dict of another node
 * (NGPU_EINVAL).  Parts whose global ids do not tile [0, entries(base)) -- an id
 * past the end or held twice -- are NGPU_EINVAL before anything is allocated. */
int ngpu_node_dict_retire_parts(ngpu_node *node, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                                uint32_t flags, ngpu_dict **out);
/* ngpu_dict_distill for node dicts (additive in ABI 7), with its contract, flags
 * and info.  A replicated dict distils every replica alike, with one result and
 * the node handle's placement rows following: the way ngpu_node_dict_retire goes
 * (out == NULL counts on the first replica alone).  A partitioned dict returns
 * NGPU_EUNSUPP from this call, as it always has: ngpu_node_dict_distill_parts
 * distils both modes.  A plain dict, or a dict of another node, is NGPU_EINVAL.
 * *out is NULL and info zeroed on every failure. */
int ngpu_node_dict_distill(ngpu_node *node, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                           ngpu_dict **out, ngpu_dict_distill_info *info);
/* ngpu_dict_distill for node dicts of both modes (additive in ABI 7).  A replicated
 * dict goes the way of ngpu_node_dict_distill.  For a partitioned dict the contract
 * is ngpu_dict_distill's, stated on the whole dict: out answers every probe, Pack,
 * ngpu_node_process_device / _step, export and save as ngpu_node_dict_create does,
 * in base's mode and exchange, over the winners of base (the first row of every
 * digest in global table order) that at least max(min_refs, 1) rows hold, in global
 * table order, with the blob rows as the flags say (the default,
 * NGPU_DICT_DISTILL_KEEP_BLOBS and NGPU_DICT_DISTILL_MERGE_BLOB_IDS mean and refuse
 * what they do for ngpu_dict_distill).  Entry ids (the global ids the parts' hits
 * carry) are positions among ALL parts' survivors; the node handle's placement rows
 * follow iff base kept them.  All rows of a digest live on one part, so every part
 * counts its own rows; a blob is live if ANY part holds a survivor in it.  Only the
 * handle's own entries(base) count: rows a later in-place extend or fold appended
 * to the parts' storages are not seen.  base is only read: probes, Packs and
 * in-place extends of it may run meanwhile.
 *
 * info is over the whole dict: entries_in = entries(base); distinct, below_min and
 * every refs_hist bucket are the sums over the parts, max_refs their maximum,
 * blobs_in and blobs_out the dict's.  It is filled on success and zeroed on every
 * failure.  out == NULL only counts: every part counts, no storage is allocated and
 * info (blobs_out included) is that of a full call.
 *
 * Every part of out sits on a storage of its own with ngpu_dict_retire's room for
 * its own survivors (s + s / 2 record slots), the node handle on placement rows
 * for all of them, so later extends and folds append in place.  A min_refs above
 * every count gives a valid dict of 0 entries and 0 blobs, which can be extended.
 * The device work runs on streams of the library's own, one per part, which
 * exchange one keep bit per entry of base between the parts (W x entries / 8 bytes
 * into every part); all parts are enqueued before the call's one mid-way wait, and
 * all streams are synchronised when the call returns, on every path.
 *
 * Rejected before any GPU work, with *out = NULL and info zeroed: a NULL node or
 * base, flag bits other than the two or both together, MERGE_BLOB_IDS on a dict
 * with records and no blob table, a plain dict, a dict of another node, parts whose
 * row counts do not add up to entries(base) (NGPU_EINVAL).  Parts whose surviving
 * global ids do not tile [0, entries(base)) -- an id past the end or held twice --
 * are NGPU_EINVAL before anything is allocated.
 *
 * UNVERIFIED ON DISTINCT GPUs, as the node exchange above: every test so far
 * lists one GPU several times. */
int ngpu_node_dict_distill_parts(ngpu_node *node, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                                 ngpu_dict **out /* NULL: count only */,
                                 ngpu_dict_distill_info *info /* may be NULL */);
/* ngpu_dict_export for node dicts of both modes (additive in ABI 7), with its
 * contract: *n_records and *n_blobs are always set, records == NULL && cap == 0
 * only counts, cap < entries(d) or too few blob_cap rows is NGPU_EINVAL with
 * nothing written.  A replicated dict goes the way of ngpu_dict_export.  For a
 * partitioned dict every part's rows come back from its device and each becomes
 * the record at the position of its global id, its compressed fields from the node
 * handle's placement row there (without placement rows: the defaults
 * ngpu_dict_export documents).  Every id must be below entries(d) and every
 * position written exactly once, else NGPU_EINVAL, and what records holds is
 * unspecified then.  flags must be 0; a plain dict or a dict of another node is
 * NGPU_EINVAL. */
int ngpu_node_dict_export(ngpu_node *node, const ngpu_dict *d, void *records, uint64_t cap,
                          uint64_t *n_records, void *blob_table, uint32_t blob_cap, uint32_t *n_blobs,
                          uint32_t flags);
int ngpu_node_dict_create(ngpu_node *node, const void *records, uint64_t n,
                          const void *blob_table, uint32_t n_blobs, uint32_t mode,
                          ngpu_dict **out);
/* ---- node dict remode: switch replicated and partitioned on the GPUs (additive in ABI 7) ----
 * out behaves exactly as ngpu_node_dict_create(node, R, B, mode) does, where R and
 * B are what ngpu_node_dict_export(base) returns: for every probe, Pack,
 * ngpu_node_process_device / _step, Check, export and save, and for every later
 * extend, fold, retire and distill.  Rows, global entry ids, blob indices, the blob
 * table (iff base has one) and the node handle's placement rows (iff base keeps
 * them) are unchanged; only where the rows live differs.  The rows never pass
 * through the host.  `mode` takes the values ngpu_node_dict_create takes, with its
 * rules: both exchange bits together is NGPU_EINVAL, ROUTED without peer access
 * falls back to the copy exchange, exchange bits on REPLICATE are ignored.
 *
 * Replicated -> partitioned (split): every part works from the replica on its own
 * device -- no peer traffic -- and keeps the rows whose digest it owns, in table
 * order, with their entry ids in base.  Partitioned -> replicated (join): every
 * replica gets all entries(base) rows, row g at position g.  The global ids are
 * walked in windows of opt->window_records ids (0: the library's default, 2^20);
 * a window is one slice per part, the other parts' slices reach the replica by
 * hipMemcpyPeerAsync into one of two staging windows (2 x window_records x 64 B per
 * replica, whatever the dict holds; (W - 1) / W x entries x 64 B cross the links per
 * replica), its own slice is read where it lies, and the first entry of a digest
 * still wins.  The same mode as base's is the compacting copy
 * ngpu_node_dict_retire_parts gives for n == 0, with the exchange `mode` asks for.
 *
 * Only the handle's own entries(base) rows count: rows a later in-place extend or
 * fold appended to the same storages are not seen.  base is only read and not
 * released: probes, Packs and in-place extends of it may run meanwhile.  Every part
 * of out sits on a storage of its own with ngpu_dict_retire's room (s + s / 2
 * record slots for its s rows), the node handle on placement rows with the same
 * room, so later extends and folds append in place.  The device work runs on
 * streams of the library's own, one per part (the join: two), outside the engine
 * locks; all of them are synchronised when the call returns, on every path.
 *
 * Rejected before any GPU work, with *out = NULL: a NULL node, base or out,
 * opt->flags or opt->reserved non-zero, a bad mode, a plain dict, a dict of another
 * node (NGPU_EINVAL).  Refused after device work, with everything freed and base as
 * it was: parts whose global ids do not tile [0, entries(base)) -- an id past the
 * end, an id held twice, a position never written (NGPU_EINVAL); an allocation
 * that fails (NGPU_ENOMEM: a join needs entries x 64 B plus the table on every GPU,
 * and the caller decides whether that fits).  Nothing a live handle can see is ever
 * written.
 * UNVERIFIED ON DISTINCT GPUs, as the node exchange above: every test so far lists
 * one GPU several times, so the join's peer copies stay inside one HBM. */
typedef struct {
  uint32_t flags;          /* reserved, 0 */
  uint32_t reserved;       /* 0 */
  uint64_t window_records; /* join: global ids per window; 0 -> the library's default */
} ngpu_node_dict_remode_options;   /* 16 bytes */
int ngpu_node_dict_remode(ngpu_node *node, ngpu_dict *base, uint32_t mode,
                          const ngpu_node_dict_remode_options *opt /* NULL: zeros */,
                          ngpu_dict **out);
/* What a node dict handle is (additive in ABI 7); touches no GPU.  A NULL argument,
 * a plain dict or a dict of another node is NGPU_EINVAL, with *out zeroed. */
typedef struct {
  uint32_t mode;              /* NGPU_NODE_DICT_PARTITION | _REPLICATE, | the exchange in use
                                 (NGPU_NODE_EXCHANGE_COPY or _ROUTED; replicated: neither) */
  uint32_t parts;             /* W */
  uint64_t entries;           /* entries(d) */
  uint64_t part_entries[64];  /* rows the handle sees on part i (replicated: entries); 0 past W */
} ngpu_node_dict_info;        /* 528 bytes */
int ngpu_node_dict_info_get(const ngpu_node *node, const ngpu_dict *d, ngpu_node_dict_info *out);
/* Device index of the node device that owns digests[32] (partitioned dicts). */
uint32_t ngpu_node_owner(const ngpu_node *node, const uint8_t *digest);
/* A Pack on the node's least-loaded engine (fewest open packs, ties round
 * robin); flags as ngpu_pack_open_dict.  ngpu_pack_engine tells which. */
int ngpu_node_pack_open(ngpu_node *node, ngpu_dict *dict, uint32_t flags, ngpu_pack **out);
int ngpu_node_process_device(ngpu_node *node, uint32_t i, ngpu_dict *dict, const void *d_data,
                             uint64_t len, const ngpu_chunk *d_chunks, uint64_t n,
                             ngpu_result *d_out, const uint64_t *d_layer_first,
                             uint64_t n_layers, ngpu_layer_stats *d_stats, void *stream);

/* ---- node step: every device at once, one all-to-all each way (ABI 5) ----
 * The bulk-synchronous form of the exchange, for a caller that converts one
 * batch of layers per device per step (C4: layers round robin over the
 * node's GPUs; convert_unix.go:467-538 runs a layer per goroutine): part i
 * (device-resident layers on node device i, its own stream there; n = 0
 * takes part with nothing) is digested, its digests are bucketed by owner
 * (ngpu_route_digests), every part's segments cross the node in ONE
 * all-to-all-v, each owner probes what it received against its partition,
 * the hits return in one all-to-all-v the other way, go back to their rows
 * and each part dedups its own layers.  Nothing in the step waits for the
 * device (ABI 5, round 5): each part's digests are bucketed into padded
 * per-owner segments of n rows, so every transfer size is known when the
 * step is enqueued, and the per-owner counts cross in band (one u32 per
 * pair) for the owners' probes to read on the device.  A caller can enqueue
 * step k+1 behind step k; the cost is W x n x 32 B out per part instead of
 * n x 32 B (csrc/a2a_plan.hpp).
 * flags NGPU_NODE_STEP_RCCL: the two all-to-alls are RCCL ncclAllToAllv
 * calls over a communicator of the node's devices (ncclCommInitAll, created on
 * the first such step; RCCL takes one rank per GPU, so a node listing a
 * device twice returns NGPU_EUNSUPP).  Without it the same segments move
 * by hipMemcpyPeerAsync (any node, also one GPU listed several times).
 * dict: a partitioned node dict (replicated or NULL: no exchange, each part
 * is processed on its own).  Returns once everything is enqueued; each
 * part's results are ready when its stream is. */
typedef struct {
  const void *d_data;             /* part's layer bytes on its device */
  uint64_t len;
  const ngpu_chunk *d_chunks;     /* n descriptors (device) */
  uint64_t n;
  ngpu_result *d_out;             /* n results (device) */
  const uint64_t *d_layer_first;  /* n_layers + 1 (device), or NULL: one layer */
  uint64_t n_layers;
  ngpu_layer_stats *d_stats;      /* device, n_layers, or NULL */
  void *stream;                   /* on the part's device (NULL: its null stream) */
} ngpu_node_part;
#define NGPU_NODE_STEP_RCCL 1u
int ngpu_node_process_step(ngpu_node *node, ngpu_dict *dict, const ngpu_node_part *parts,
                           uint32_t n_parts, uint32_t flags);

/* ---- RAFS v6 chunk table ---------------------------- */
/* Serialise the layer's unique chunk records (NEW chunks in index order) as
 * 80-byte RAFS v6 chunk-info entries.  compressor "none": compressed size =
 * uncompressed size, compressed offsets packed back to back.  `blob_index`
 * of each record is the result's real blob index.  Writes at most cap
 * records; *n_records receives the count. */
int ngpu_chunk_table(const ngpu_chunk *chunks, const ngpu_result *results,
                     uint64_t n, uint8_t *out /* cap x 80 */, uint64_t cap,
                     uint64_t *n_records);

/* ---- nydus blob stream: converter.Pack's output --
 * The stream nydus-image writes for `--type tar-rafs --blob-inline-meta
 * --features blob-toc` (builder.go:97-110) and packFromTar copies to `dest`
 * (convert_unix.go:486-495): `data | tar_header | ... | toc | tar_header`
 * (convert_unix.go:296-300).  Entries: image.blob (the layer's NEW chunks in
 * index order, each compressed on its own, raw when compression does not
 * shrink it), image.boot (the RAFS v6 -- or, FsVersion 5, v5 -- bootstrap of
 * the layer: the tar's whole inode tree, every regular file's chunks, blob
 * table, prefetch table, and the chunk table: one record per distinct chunk
 * the layer references -- its NEW chunks and the chunk-dict chunks it reuses,
 * copied with their dict blob placement),
 * blob.meta + blob.meta.header (convert_unix.go:47-48: the chunk-info array
 * of the layer's blob and its 4 KiB header) and blob.digest (the chunks'
 * digests, index order) when the blob has chunks, and
 * rafs.blob.toc (128-B TOCEntry records, types.go:147-163).  Compression and
 * SHA-256 run on the host (north star: compression stays on the host path). */

/* PackOption.Compressor / TOCEntry.Flags values (types.go:22-31). */
enum ngpu_compressor {
  NGPU_COMPRESSOR_NONE = 0x1,
  NGPU_COMPRESSOR_ZSTD = 0x2,
  NGPU_COMPRESSOR_LZ4_BLOCK = 0x4
};

/* io.Writer: return 0 after consuming all len bytes, non-zero on error. */
typedef int (*ngpu_write_fn)(void *ctx, const void *buf, uint64_t len);
/* content.ReaderAt: bytes read (> 0) or a negative error. */
typedef int64_t (*ngpu_read_at_fn)(void *ctx, void *buf, uint64_t len, uint64_t off);

typedef struct {
  uint32_t compressor;   /* enum ngpu_compressor; 0 -> zstd */
  int32_t level;         /* compressor level; 0 -> library default (zstd: 1) */
  uint32_t threads;      /* host compression threads; 0 -> min(16, cores) */
  uint32_t digester;     /* ngpu_blob_write only: bootstrap digest flag */
  uint32_t chunk_size;   /* ngpu_blob_write only: bootstrap chunk size */
  uint32_t n_dict_blobs; /* records in dict_blobs */
  const uint8_t *dict_blobs; /* the chunk dict's blob table (n x 256-B RAFS v6
                                blob records, inner-index order), or NULL;
                                ngpu_pack_finish defaults to the blob table of
                                the pack's dict */
  const void *dict_chunks;   /* ngpu_blob_write: the chunk dict's chunk table
                                (80-B RAFS v6 records, entry order) the DICT
                                results' `ref` index, for the compressed
                                placement their records copy; NULL: csize =
                                usize, offset 0.  ngpu_pack_finish uses the
                                pack's dict */
  uint64_t n_dict_chunks;
  uint32_t fs_version;       /* ngpu_blob_write only: PackOption.FsVersion 5 or 6
                                (0 -> 6); ngpu_pack_finish uses the engine's.  v6:
                                RAFS v6 image.boot + blob.meta + TOC (`--features
                                blob-toc`, builder.go:104-110); v5: RAFS v5
                                image.boot, no TOC */
  uint32_t reserved;
  const char *prefetch_patterns; /* PackOption.PrefetchPatterns: newline-separated
                                paths (the builder's stdin, builder.go:125-127,
                                166); NULL or "" -> "/" */
} ngpu_blob_options;

typedef struct {
  uint64_t stream_bytes;      /* bytes written to dest */
  uint64_t blob_bytes;        /* image.blob: compressed chunk data */
  uint64_t bootstrap_bytes;   /* image.boot */
  uint64_t blob_chunks;       /* chunk records of the layer's own blob (NEW) */
  uint64_t compressed_chunks; /* of which stored compressed */
  uint8_t stream_digest[32];  /* sha256 of the whole stream: the layer blob
                                 digest (LayerConvertFunc, convert_unix.go:870-914) */
  uint8_t blob_digest[32];    /* sha256 of image.blob (the own blob's id) */
  uint8_t toc_digest[32];     /* sha256 of the TOC (calcBlobTOCDigest :541-555) */
  uint64_t dict_records;      /* chunk records copied from the chunk dict */
  uint64_t meta_entries;      /* entries of the blob.meta chunk-info array (0: none) */
} ngpu_blob_info;

/* Thread-local message of the last failing engine-less call below. */
const char *ngpu_host_error(void);
/* A ready-made ngpu_write_fn: ctx is a file descriptor ((void *)(intptr_t)fd). */
int ngpu_write_fd(void *ctx, const void *buf, uint64_t len);

/* ---- dict save: a dict handle written out as a RAFS v6 dict bootstrap (additive
 * in ABI 7) ----
 * The handle's records and blob rows go to `w` as the chunk-table-only RAFS v6
 * bootstrap that ngpu_dict_open, ngpu_dict_extend_bootstrap, ngpu_merge* and
 * inspect read: bytes [0, 4096) are zero but for the super block magic at 1024
 * and, at 1152, flags (u64: 0x4 blake3, 0x8 sha256, the handle's digester),
 * blob_table_offset (u64: 4096, or 0 without blob rows), blob_table_size (u32:
 * 256 x b), chunk_size (u32), chunk_table_offset (u64: 4096 + 256 x b rounded up
 * to 4096), chunk_table_size (u64: 80 x k), prefetch offset and size (0).  The
 * handle's 256-B blob rows follow at 4096 as it holds them, zero padded to the
 * chunk table; then the k records ngpu_dict_export returns for entries
 * [first_entry, entries), with blob_index - first_blob.
 *
 * The records are made on the device, a window at a time: the window's placement
 * rows go up (a dict that keeps them), one kernel writes the 80-B records, one
 * copy brings them into pinned memory and `w` gets them as they are, from the
 * calling thread, in file order, while the next window is on its way.  Host
 * memory is two windows (window_records records each; 0: what one staging slot of
 * the engine holds), whatever the dict's size.  The engine lock is not held; the
 * call reads only the handle's own rows, so probes and in-place extends of the
 * same storage may run meanwhile, and so may another save.
 *
 * Range save: first_entry = entries(h0) and first_blob = blobs(h0) of a handle h0
 * that d descends from by extends and folds write only what came after h0, shaped
 * as ngpu_dict_extend_bootstrap takes it: open(file(h0)) extended by that file
 * exports what d exports.
 *
 * Refused before `w` is called, with *info zeroed (NGPU_EINVAL unless said):
 * a NULL dict, engine / node or writer; unknown flags or a non-zero reserved word;
 * first_entry > entries(d) or first_blob > blobs(d); a record in the range whose
 * blob index is below first_blob (d does not descend from h0 by extends, e.g.
 * after a retire; one launch over the range finds it, only when first_blob > 0;
 * the message names the first such entry); a handle that holds records and a blob
 * count but no blob table, unless NGPU_DICT_SAVE_NO_BLOB_TABLE is set: the file
 * then carries no blob table and reopening it counts max(blob_index) + 1 blobs,
 * which is less than blobs(d) when d's last blobs hold no record.  ngpu_dict_save
 * takes plain dicts and replicated node dicts (part 0's rows); for a partitioned
 * node dict it returns NGPU_EUNSUPP: ngpu_node_dict_save takes both node modes (a
 * plain dict there is NGPU_EINVAL).  Two windows the engine's pool cannot give
 * are NGPU_ENOMEM.  A writer that fails gives NGPU_EIO: the stream is drained,
 * both windows go back to the pool and the engine's counters read as before.
 *
 * A partitioned node dict: every part's rows lie in ascending global id order.
 * Per window [a, b) each part's slice (found by one lower-bound launch per part
 * for all the cuts) is copied to node device 0 and a scatter form of the kernel
 * writes row g to slot g - a.  Rows outside [a, b), a slot written twice or slices
 * that do not add up to b - a are NGPU_EINVAL ("the parts do not tile the dict's
 * ids"), possibly after earlier windows were written. */
#define NGPU_DICT_SAVE_NO_BLOB_TABLE 0x1u
typedef struct {
  uint64_t first_entry;     /* 0, or entries() of an ancestor handle that was saved before */
  uint32_t first_blob;      /* 0, or that handle's blob count */
  uint32_t flags;
  uint64_t window_records;  /* records per window; 0: the library's default */
  uint64_t reserved[2];     /* must be 0 */
} ngpu_dict_save_options;   /* 40 bytes */
typedef struct {
  uint64_t entries, blobs;  /* records and blob rows written */
  uint64_t bytes;           /* the whole file */
  uint64_t blob_table_offset, blob_table_size, chunk_table_offset, chunk_table_size;
  uint64_t windows;
} ngpu_dict_save_info;      /* 64 bytes */
/* The layout of a file of `entries` records and `blobs` blob rows (windows = 0);
 * host only, no engine.  NGPU_EINVAL past ngpu_dict_create's limits. */
int ngpu_dict_save_layout(uint64_t entries, uint32_t blobs, ngpu_dict_save_info *out);
int ngpu_dict_save(ngpu_engine *eng, const ngpu_dict *d, const ngpu_dict_save_options *opt /* NULL: zeros */,
                   ngpu_write_fn w, void *ctx, ngpu_dict_save_info *info /* may be NULL */);
int ngpu_node_dict_save(ngpu_node *node, const ngpu_dict *d, const ngpu_dict_save_options *opt,
                        ngpu_write_fn w, void *ctx, ngpu_dict_save_info *info);

/* Host: write the stream of one packed layer whose bytes are in host memory
 * (chunks/results/stats as returned by ngpu_pack_tar).  `data` must be the
 * layer tar the chunks were cut from: its entries are the bootstrap's inode
 * tree (NGPU_EINVAL when walking it does not give `chunks`). */
int ngpu_blob_write(const void *data, uint64_t len, const ngpu_chunk *chunks,
                    const ngpu_result *results, uint64_t n, const ngpu_layer_stats *stats,
                    const ngpu_blob_options *opt, ngpu_write_fn w, void *ctx,
                    ngpu_blob_info *info);

/* Streaming Pack that writes the stream at the end: NGPU_PACK_RETAIN keeps the
 * layer bytes in HBM (288 GB) instead of recycling the device slots, so that
 * ngpu_pack_finish can gather the NEW chunks on the GPU, copy only those to
 * the host and compress them.  ngpu_pack_finish = ngpu_pack_close + stream
 * (releases the pack in every case). */
#define NGPU_PACK_RETAIN 0x1u
/* PackOption.OCIRef (ABI 4; `nydus-image create --type targz-ref`,
 * builder.go:180-218): ngpu_pack_write takes the ORIGINAL gzip layer blob.  The
 * library inflates it on the host (one gzip member), the tar stream takes the
 * tar-rafs path (tar walk, GPU digests, layered dedup; no chunk dict, as
 * packRef passes none), and a checkpoint of the deflate stream is kept every
 * max(chunk size, 1 MiB) of output.  The output stream holds no image.blob:
 * blob.meta (chunk-info array with each chunk's checkpoint, the checkpoint
 * table and the 32 KiB dictionaries), blob.digest, image.boot and the TOC; the
 * bootstrap's own blob is the gzip blob (id = its sha256, the digest Merge
 * returns for the layer, converter_test.go TestPackRef), each chunk record
 * carrying the deflate range that produces it.
 * EXPERIMENTAL: the blob.meta zran layout (ZranInflateContext records, the
 * zran header words, super flag 0x40, the chunk entry's data word) is
 * restated from nydus v2.3.0 and NOT pinned by any reference fixture; this
 * library's own reader (ngpu_ref_chunk_read) round-trips it, nydusd has not
 * read it.  A chunk whose deflate range or checkpoint offset does not fit its
 * field (24-bit size, 40-bit offset, 32-bit offsets) fails with NGPU_EFORMAT,
 * never truncated.  ngpu_pack_reserve / ngpu_pack_commit are not available
 * (EINVAL). */
#define NGPU_PACK_OCIREF 0x2u
/* The reader side of an OCIRef layer (host; what nydusd does with a targz-ref
 * blob): chunk `index` of the layer's own blob, located through `blob_meta`
 * (the layer stream's blob.meta tar entry: chunk-info array, checkpoint table,
 * dictionaries, then the 4 KiB header -- through the TOC, the "blob.meta"
 * entry followed by "blob.meta.header") and inflated out of the original gzip blob `gz` from
 * its checkpoint.  *len_out = the chunk's size (<= cap).  (ABI 4) */
int ngpu_ref_chunk_read(const void *gz, uint64_t gz_len, const void *blob_meta, uint64_t meta_len,
                        uint32_t index, void *out, uint32_t cap, uint32_t *len_out);
int ngpu_pack_open_ex(ngpu_engine *eng, uint32_t flags, ngpu_pack **out);
int ngpu_pack_finish(ngpu_pack *p, const ngpu_blob_options *opt, ngpu_write_fn w, void *ctx,
                     ngpu_chunk **chunks_out, ngpu_result **results_out, uint64_t *n_out,
                     ngpu_layer_stats *stats, ngpu_blob_info *info);
/* Early emission (ABI 4): give a NGPU_PACK_RETAIN pack its output before the
 * first write (converter.Pack knows `dest` when it opens, convert_unix.go:325).
 * An emitter thread then writes the blob stream while the tar is still
 * arriving: after each staging slot is digested it dedups the prefix so far
 * (a chunk's decision depends only on the chunks before it) and compresses,
 * hashes and writes the NEW chunks that became final, so the sequential host
 * SHA-256 of the stream overlaps the copies and digests of the rest of the
 * layer.  Finish with ngpu_pack_finish(p, NULL, NULL, NULL, ...): it writes the
 * rest, image.boot and the TOC.  The bytes are the same as with a writer given
 * to ngpu_pack_finish.  `opt` is copied (prefetch_patterns too); dict_blobs /
 * dict_chunks must stay valid until finish.  w is called from the library's
 * threads.  An emitter error fails the next write and the finish. */
int ngpu_pack_set_output(ngpu_pack *p, const ngpu_blob_options *opt, ngpu_write_fn w, void *ctx);

/* UnpackEntry (convert_unix.go:284-320): find `name` through the TOC
 * (seekFileByTOC :219-276; entry compressor none or zstd), else by walking
 * the tar headers from the tail (seekFileByTarHeader :162-213), and copy its
 * data to w.  toc_entry_out (128 B, may be NULL) receives the TOC entry, or
 * zeros when found by tar header.  NGPU_ENOTFOUND = ErrNotFound. */
int ngpu_unpack_entry(ngpu_read_at_fn ra, void *ctx, uint64_t size, const char *name,
                      ngpu_write_fn w, void *wctx, uint8_t *toc_entry_out);

/* Unpack (convert_unix.go:669-719, `nydus-image unpack`): the nydus stream of
 * a packed layer (read through ra, `size` bytes) back to an OCI tar written to
 * w: image.boot's inode tree depth first in name order, each regular file's
 * chunks read from image.blob and decompressed.  Headers use the Go
 * archive/tar USTAR encoding (PAX records where USTAR cannot hold a value),
 * user / group names from the host's passwd / group; a hardlinked inode is a
 * file at its first path and a hardlink ('1') at the others.  A chunk in
 * another blob (a chunk-dict blob) is NGPU_ENOTFOUND: only the layer's own
 * blob travels in its stream. */
int ngpu_unpack(ngpu_read_at_fn ra, void *ctx, uint64_t size, ngpu_write_fn w, void *wctx);

/* ---- Check: re-digest a converted layer's chunks (additive in ABI 7) --------
 * The reference proves a conversion by reading it back: `nydusify check`
 * closes TestImageConvert (tests/converter_test.go:865-875) and nydusd
 * validates chunk digests when it serves them (`digest_validate`,
 * tests/nydusd.go:69).  Here: every chunk record of a bootstrap is read from
 * its blob, inflated on the host, hashed again on the GPU and compared with the
 * record's block_id.
 *
 * ngpu_check_device: the device stage, device pointers, async on `stream`
 * (no host wait).  The digest stage of ngpu_digest_device into d_out, then
 * the verdict kernel: bit i % 64 of d_bitmap[i / 64] is set iff d_out[i].kind
 * != NGPU_DIGESTED or the 32 digest bytes differ from d_expected + i *
 * expected_stride.  d_counts[0] = set bits, d_counts[1] = how many of them
 * were not NGPU_DIGESTED.  The call writes every one of the (n + 63) / 64
 * bitmap words (zero words and the zero tail bits of the last one included)
 * and zeroes d_counts itself on `stream`: the caller clears nothing.
 * expected_stride >= 32 and a multiple of 4, d_expected 4-byte aligned
 * (NGPU_EINVAL otherwise); 16-byte loads when d_expected and the stride are
 * 16-byte aligned -- 32, or 80 to read the block_id of RAFS v6 chunk-info
 * records in place -- dword loads otherwise.  n == 0 only zeroes the counts;
 * n >= 0xFFFFFFFF is NGPU_EINVAL.  Locking and workspace use as
 * ngpu_digest_device. */
int ngpu_check_device(ngpu_engine *eng, const void *d_data, uint64_t len,
                      const ngpu_chunk *d_chunks, uint64_t n, ngpu_result *d_out,
                      const uint8_t *d_expected, uint64_t expected_stride,
                      uint64_t *d_bitmap /* (n + 63) / 64 words */,
                      uint64_t *d_counts /* 2 words */, void *stream);

/* A blob offered to ngpu_check_image: `id` is the blob id in the bootstrap's
 * blob table (64 hex chars); the reader is the blob's chunk data (image.blob)
 * or a whole layer stream -- a record's compressed_offset counts from offset
 * 0 in both.  ra may be called from several threads at once (content.ReaderAt
 * allows it). */
typedef struct {
  const char *id;
  ngpu_read_at_fn ra;
  void *ctx;
  uint64_t size;
} ngpu_check_blob;
typedef struct {
  uint32_t flags;        /* reserved, 0 */
  uint32_t threads;      /* host inflate threads; 0 -> min(16, cores) */
  uint64_t window_bytes; /* staging window; 0 -> the engine's staging_bytes */
} ngpu_check_options;
typedef struct {
  uint64_t records;      /* distinct chunk records of the bootstrap */
  uint64_t checked;      /* read from a supplied blob and compared (bad ones included) */
  uint64_t bad;          /* failures of any reason, listed or not */
  uint64_t dict_checked; /* records of blobs not supplied, resolved in the dict */
  uint64_t dict_bad;     /* of which NGPU_CHECK_DICT failures (counted in bad too) */
  uint64_t skipped;      /* records of blobs not supplied, no dict given */
  uint64_t bytes;        /* uncompressed bytes hashed on the GPU */
} ngpu_check_report;
enum {
  NGPU_CHECK_DIGEST = 1,     /* the chunk's bytes do not hash to its block_id */
  NGPU_CHECK_DECOMPRESS = 2, /* the chunk does not inflate to its uncompressed size */
  NGPU_CHECK_RANGE = 3,      /* compressed range outside the blob, or an uncompressed
                                size of 0 or above the chunk size */
  NGPU_CHECK_DICT = 4        /* not resolved by the chunk dict */
};
typedef struct {
  uint32_t blob_index, index, reason, uncompressed_size; /* the record's fields + why */
  uint64_t compressed_offset;
  uint8_t expected[32]; /* the record's block_id */
  uint8_t got[32];      /* NGPU_CHECK_DIGEST: the digest of the bytes read; else zeros */
} ngpu_check_bad;

/* Check every distinct chunk record of a RAFS v6 bootstrap (its chunk table,
 * table order) or v5 bootstrap (distinct (blob, index) over the regular files'
 * chunks, inode-table order) once.  A record whose blob is among `blobs`
 * (matched by id) is bounds-checked against the blob's size, inflated with the
 * blob's compressor on `threads` host threads (copied when stored raw) into a
 * pinned window, copied to HBM and run through ngpu_check_device beside its
 * expected digest; only the bitmap and counts come back, and the results of
 * windows that hold a bad record.  The host fills one window while the GPU
 * works on the other.  A record whose blob is not supplied is looked up in
 * `dict` on the GPU (an engine or node dict; NULL: counted as skipped): it is
 * NGPU_CHECK_DICT-bad unless the dict holds its digest with a matching size
 * (dict usize 0 or equal) at the same chunk index and uncompressed offset in
 * a blob of the same id.
 * report->bad counts every failure; bad[0 .. min(bad, bad_cap)) lists the
 * first ones in record order.  A failing record never stops the check.
 * Returns 0 when the check ran to its end (read the report); NGPU_EINVAL: the
 * bootstrap's digester or chunk size is not the engine's, or window_bytes is
 * below the chunk size; NGPU_EUNSUPP: a targz-ref (OCIRef) bootstrap;
 * NGPU_EFORMAT: a malformed bootstrap; NGPU_EIO: a reader failed inside a
 * range it claimed to hold; NGPU_EDEVICE: the digest stage left records
 * unhashed.  Untrusted input: every size is bounded before it sizes a buffer. */
int ngpu_check_image(ngpu_engine *eng, const void *bootstrap, uint64_t size,
                     const ngpu_check_blob *blobs, uint32_t n_blobs, ngpu_dict *dict,
                     const ngpu_check_options *opt, ngpu_check_report *report,
                     ngpu_check_bad *bad, uint64_t bad_cap);
/* The same for one packed layer's nydus stream: image.boot is found as
 * ngpu_unpack finds it, and the stream's image.blob is offered as the layer's
 * own blob (ngpu_unpack's rule: the blob named by image.blob's TOC digest,
 * else the one of its size).  Like ngpu_unpack it trusts the TOC for
 * locations and does not verify the TOC's entry digests. */
int ngpu_check_stream(ngpu_engine *eng, ngpu_read_at_fn ra, void *ctx, uint64_t size,
                      ngpu_dict *dict, const ngpu_check_options *opt, ngpu_check_report *report,
                      ngpu_check_bad *bad, uint64_t bad_cap);

/* ---- Verity: the dm-verity hash tree of a block image (additive in ABI 7) ---
 * tarfs's `nydus-image export --block --verity` appends a dm-verity hash tree
 * to the exported disk image and prints the options that open it
 * (pkg/tarfs/tarfs.go:548: --no-superblock --format=1 -s "" --hash=sha256
 * --data-block-size=512 --hash-block-size=4096 --data-blocks N --hash-offset
 * OFF ROOT).  Exactly that tree, as cryptsetup and the kernel's dm-verity
 * define it: a digest is SHA-256 of a whole 512-byte data block or a whole
 * 4096-byte hash block (empty salt); a hash block is up to 128 consecutive
 * digests of the level below, zero padded; level i (0 = above the data) has
 * ceil(data_blocks / 128^(i+1)) hash blocks; `levels` is the smallest L >= 0
 * with (data_blocks - 1) >> (7 L) == 0; the tree is the levels top first,
 * level 0 last; the root is the SHA-256 of the single top hash block, or of
 * the one data block when levels == 0 (tree_bytes == 0 then).  Only the tree:
 * the block image itself (`export --block`) is not produced here. */
typedef struct {
  uint64_t data_blocks; /* data_bytes / 512 */
  uint64_t hash_offset; /* data_bytes rounded up to 4096: where the tree goes in the image file */
  uint64_t tree_bytes;  /* 4096 x hash blocks of all levels */
  uint32_t levels;
  uint32_t reserved;
  uint8_t root[32];     /* ngpu_verity_layout leaves it zero */
} ngpu_verity_info;

/* The geometry alone; no engine, no GPU.  NGPU_EINVAL unless data_bytes is a
 * non-zero multiple of 512 below 2^62. */
int ngpu_verity_layout(uint64_t data_bytes, ngpu_verity_info *out);

/* The device stage: device pointers, async on `stream`, no host wait.  d_tree
 * receives the tree_bytes of ngpu_verity_layout(data_bytes) -- every byte,
 * the zero tail of each level's last hash block included: the caller clears
 * nothing -- and d_root the 32-byte root.  One launch for the data blocks,
 * one per level above them, one for the root.  d_data and d_tree must be
 * 16-byte aligned (NGPU_EINVAL otherwise, and for a bad data_bytes); d_tree
 * may be NULL when tree_bytes is 0.  The tree is always SHA-256, whatever the
 * engine's digester; no workspace is used, and the engine lock is held for the
 * enqueue only. */
int ngpu_verity_device(ngpu_engine *eng, const void *d_data, uint64_t data_bytes, void *d_tree,
                       void *d_root, void *stream);

typedef struct {
  uint32_t flags;        /* reserved, 0 */
  uint32_t threads;      /* host reader threads; 0 -> min(16, cores) */
  uint64_t window_bytes; /* staging window, rounded down to a multiple of 512;
                            0 -> the engine's staging_bytes */
} ngpu_verity_options;

/* The host pipeline: the image's first data_bytes are read through `ra` (from
 * several threads at once) into two pinned windows of the engine's staging
 * pool, copied to HBM and hashed into the level-0 region of a tree kept in
 * HBM while the host fills the other window; the upper levels run after the
 * last window, and the tree comes back through the pinned windows and is
 * handed to `w` in order (w may be NULL: only *info is wanted).  Returns with
 * everything it took released.  NGPU_EINVAL: a bad data_bytes, or a window
 * below 512 bytes; NGPU_EIO: the reader failed (or `w` did); NGPU_ENOMEM: the
 * tree or the windows do not fit. */
int ngpu_verity_image(ngpu_engine *eng, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                      const ngpu_verity_options *opt, ngpu_write_fn w, void *wctx,
                      ngpu_verity_info *info);

/* ---- Verity verify: an image against its STORED tree (additive in ABI 7) ----
 * What the kernel's dm-verity and `veritysetup verify` decide, for every block
 * at once and with a verdict per block.  The inputs are the data, the stored
 * tree and a trusted 32-byte root; the geometry is ngpu_verity_layout's and
 * comes from data_bytes alone -- nothing read from the image sizes or
 * addresses anything.  With first[l] the tree block at which level l starts:
 *   - data block i is bad iff SHA-256 of its 512 bytes differs from the 32
 *     stored bytes at tree offset first[0] * 4096 + 32 i (levels == 0: from
 *     the root);
 *   - tree block t = first[l] + j has a bad hash iff SHA-256 of its 4096
 *     stored bytes differs from the 32 stored bytes at first[l + 1] * 4096 +
 *     32 j; the top block (t == 0) is compared with the root;
 *   - level l has a bad spare area iff a byte of its last hash block after
 *     that block's last digest is not zero (libcryptsetup refuses such a
 *     tree, "Spare area is not zeroed", even when every hash is consistent).
 * The image verifies iff none occurs, which holds iff the rebuilt tree equals
 * the stored one and its root is the given root.  Every stored block is
 * checked against its stored parent, so no level waits for another and a
 * finding stays where the damage is: one flipped data byte is one bad data
 * block and no bad hash block; a flipped byte in digest slot s of level-0
 * block j is tree block first[0] + j (bad hash) and data block 128 j + s.
 *
 * The device calls: device pointers, async on `stream`, no host wait, no
 * workspace, the engine lock held for the enqueue only.  d_data and d_tree
 * must be 16-byte aligned, bitmaps and counts 8-byte aligned; `root` is host
 * memory, read before the call returns; d_tree may be NULL when tree_bytes is
 * 0.  Every word of a bitmap is written (zero words and the zero tail bits of
 * the last word too: the caller clears nothing), and the counts are zeroed on
 * `stream` first.  NGPU_EINVAL, with nothing launched: a misaligned or missing
 * pointer, a bad data_bytes, first_block + n_blocks above data_blocks, or more
 * blocks than one launch takes.  n_blocks == 0, or a tree call when
 * tree_bytes is 0, only zeroes the counts. */

/* All stored hash blocks of all levels in one launch: bit t of word t / 64 is
 * set iff tree block t has a bad hash. */
int ngpu_verity_verify_tree_device(ngpu_engine *eng, uint64_t data_bytes, const void *d_tree,
                                   const uint8_t root[32] /* host */,
                                   uint64_t *d_tree_bitmap /* (tree_blocks + 63) / 64 words */,
                                   uint64_t *d_counts /* [0] bad-hash blocks, [1] spare mask: bit l = level l */,
                                   void *stream);
/* Data blocks [first_block, first_block + n_blocks) of the image, at d_data,
 * against the stored level 0 in d_tree (the whole tree, as stored): bit k of
 * word k / 64 is set iff data block first_block + k is bad. */
int ngpu_verity_verify_data_device(ngpu_engine *eng, const void *d_data, uint64_t first_block,
                                   uint64_t n_blocks, uint64_t data_bytes, const void *d_tree,
                                   const uint8_t root[32] /* host */,
                                   uint64_t *d_bitmap /* (n_blocks + 63) / 64 words, window-relative */,
                                   uint64_t *d_count /* 1 word */, void *stream);

typedef struct {
  uint64_t data_blocks, tree_blocks, levels;
  uint64_t bad_data;  /* bad data blocks */
  uint64_t bad_hash;  /* tree blocks with a bad hash */
  uint64_t bad_spare; /* levels with a bad spare area */
  uint64_t bad;       /* all findings, listed or not: the image verifies iff 0 */
  uint64_t bytes;     /* data and tree bytes hashed on the GPU */
} ngpu_verity_report;
enum {
  NGPU_VERITY_BAD_DATA = 1, /* a data block does not hash to its stored level-0 digest */
  NGPU_VERITY_BAD_HASH = 2, /* a stored hash block does not hash to its stored parent digest / the root */
  NGPU_VERITY_BAD_SPARE = 3 /* the spare area of a level's last hash block is not zero */
};
typedef struct {
  uint32_t reason;
  uint32_t level;            /* of a tree block (0 = above the data); 0 for a data block */
  uint64_t block;            /* the data-block number, or the tree-block number */
  uint64_t first_data_block; /* the data blocks it covers, inclusive; */
  uint64_t last_data_block;  /* for a data block, the block itself */
  uint64_t file_offset;      /* 512 * block, or hash_offset + 4096 * block */
} ngpu_verity_bad;

/* The host pipeline, shaped like ngpu_verity_image.  The stored tree is read
 * from hash_offset through the pinned windows into HBM and checked in one
 * launch; then the image's first data_bytes follow window by window (H2D, one
 * launch against the tree in HBM) while the host fills the other window.  Only
 * each window's bitmap and count come back, and the host scans a bitmap only
 * when its count is not zero.  report->bad counts every finding;
 * bad[0 .. min(bad, bad_cap)) lists the first ones in this order: tree
 * findings in tree-block order (top first; a block's HASH entry before its
 * SPARE entry), then data blocks ascending.  A finding never stops the run:
 * 0 means it ran to its end (read the report).  Returns with everything it
 * took released.  NGPU_EINVAL: a bad data_bytes, a window below 512 bytes,
 * hash_offset below data_bytes, or hash_offset + tree_bytes wrapping;
 * NGPU_EIO: the reader failed, a file that ends before the tree does included;
 * NGPU_ENOMEM: the tree or the windows do not fit. */
int ngpu_verity_verify_image(ngpu_engine *eng, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                             uint64_t hash_offset, const uint8_t root[32],
                             const ngpu_verity_options *opt, ngpu_verity_report *report,
                             ngpu_verity_bad *bad, uint64_t bad_cap);

/* converter.Merge (convert_unix.go:560-666) -> tool.Merge (builder.go:220-294,
 * `nydus-image merge --prefetch-policy fs [--chunk-dict] [--parent-bootstrap]`):
 * per-layer bootstraps (the image.boot entries, lowest layer first) into the
 * image's bootstrap, written to w in the layers' RAFS version (v5 or v6; all
 * layers must share it and the chunk size).  The inode trees are overlaid
 * with the OCI layer rules: an upper entry replaces the lower one of its path,
 * directories merge, `.wh.<name>` removes <name> and its subtree from the
 * layers below, `.wh..wh..opq` hides everything below its directory, and the
 * whiteouts themselves are dropped.  Chunk records keep their placement; their
 * blob indices point into the merged blob table.  A layer's own blob (any
 * blob not in the chunk dict bootstrap's blob table) is named
 * layer_digests[l] (hex of Layer.Digest, the bootstrap file name the
 * reference passes to nydus-image merge); at most one per layer.
 * *blob_ids_out (malloc'd, ngpu_free_host) = comma-separated blob ids in
 * first-appearance order (the output JSON's "Blobs"). */
int ngpu_merge(const void *const *bootstraps, const uint64_t *sizes,
               const char *const *layer_digests, uint64_t n, const void *dict_bootstrap,
               uint64_t dict_size, ngpu_write_fn w, void *ctx, char **blob_ids_out);

/* `nydus-image inspect`, restated (north_star: bootstraps "compared via
 * nydus-image inspect"): one JSON object for a RAFS
 * v5 or v6 bootstrap, written to w --
 *   {"fs_version", "chunk_size", "flags", "blobs": [{"id", "chunk_count",
 *    "compressed_size", "uncompressed_size"}], "inodes": [{"path" ("/" first,
 *    then depth first in name order), "mode", "uid", "gid", "size", "nlink",
 *    "ino", "rdev", "mtime", "mtime_ns", "link" (symlinks), "xattrs" (name ->
 *    hex value), "chunks": [[digest hex, blob index, flags, compressed
 *    offset, compressed size, uncompressed offset, uncompressed size, file
 *    offset, chunk index], ...]}]}
 * Bytes outside printable ASCII in names are \u00XX escapes (latin-1).
 * Untrusted input: bounds-checked (NGPU_EFORMAT). */
int ngpu_rafs_dump(const void *bootstrap, uint64_t size, ngpu_write_fn w, void *ctx);

/* MergeOption fields beyond the chunk dict (types.go:92-133). */
typedef struct ngpu_merge_options {
  /* ParentBootstrapPath's contents (--parent-bootstrap): the lowest layer,
   * its blobs keep their ids (any number of them); NULL = none */
  const void *parent_bootstrap;
  uint64_t parent_size;
  /* PrefetchPatterns (the builder's stdin, builder.go:238-240, 269):
   * newline-separated paths; NULL or "" = "/" */
  const char *prefetch_patterns;
  /* (ABI 6 appended the targz-ref arrays here; ABI 7 takes them as arguments
   * of ngpu_merge_ex2 instead, so a caller built against either header passes
   * a struct this library reads no further than its end.) */
} ngpu_merge_options;

/* ngpu_merge with MergeOption's parent bootstrap and prefetch patterns
 * (opt may be NULL: ngpu_merge). */
int ngpu_merge_ex(const void *const *bootstraps, const uint64_t *sizes,
                  const char *const *layer_digests, uint64_t n, const void *dict_bootstrap,
                  uint64_t dict_size, const ngpu_merge_options *opt, ngpu_write_fn w, void *ctx,
                  char **blob_ids_out);
/* ngpu_merge_ex with targz-ref layers (ABI 7; Layer.OriginalDigest:
 * convert_unix.go:577-590 hands nydus-image --blob-digests / --blob-sizes /
 * --blob-toc-digests, builder.go:242-253).  The three arrays are NULL (no
 * targz-ref layer) or n entries each, entry l NULL / ignored for a layer
 * without OriginalDigest: 64 hex chars of the layer's RAFS blob (its nydus
 * stream) digest, its size, and 64 hex chars of the sha256 of its TOC entry
 * data (calcBlobTOCDigest, convert_unix.go:541-554).  Recorded in the layer's
 * own blob record of the merged bootstrap (RafsV6Blob blob_toc_digest /
 * blob_meta_digest / blob_meta_size; offsets restated from nydus v2.3.0,
 * parity unpinned). */
int ngpu_merge_ex2(const void *const *bootstraps, const uint64_t *sizes,
                   const char *const *layer_digests, uint64_t n, const void *dict_bootstrap,
                   uint64_t dict_size, const ngpu_merge_options *opt,
                   const char *const *rafs_blob_digests, const uint64_t *rafs_blob_sizes,
                   const char *const *rafs_blob_toc_digests, ngpu_write_fn w, void *ctx,
                   char **blob_ids_out);

#ifdef __cplusplus
}
#endif
#endif /* NYDUS_GPU_H */
