// check.hip — Check: re-digest the chunks of a converted layer and compare
// them with the digests its bootstrap records (include/nydus_gpu.h, "Check").
//
// The reference proves a conversion by reading it back (`nydusify check` at
// the end of TestImageConvert, tests/converter_test.go:865-875; nydusd's
// `digest_validate`, tests/nydusd.go:69).  Here:
//   * check_digests: the verdict kernel.  One lane per record compares the 32
//     digest bytes the digest stage wrote with the expected ones; one
//     __ballot per wave64 gives the record's bitmap word, which lane 0 stores
//     whole (zero words too: the caller never clears the bitmap), and a
//     non-zero word adds its popcount to the counters with one atomicAdd.
//     Only a wave with a non-zero word takes a second ballot, of the records
//     the digest stage left unhashed, and a second atomicAdd if there are any
//     (the error path).
//   * ngpu_check_image: the host pipeline (window_bufs.hpp, host_window.hpp).
//     The bootstrap's chunk records are cut into windows of whole chunks
//     (check_plan.hpp); the reader pool reads each chunk from its blob and
//     inflates it into a pinned window, the window goes to HBM with its chunk
//     list and expected digests, and only the bitmap + counters come back --
//     the results too for a window with a bad record, to report the digest
//     found.
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "check_plan.hpp"
#include "host_window.hpp"
#include "window_bufs.hpp"

namespace ngpu {
namespace {

// VEC: d_out and the expected digests are 16-byte aligned (base and stride):
// two 16-B loads a side; otherwise eight dword loads of the expected digest.
template <bool VEC>
__global__ __launch_bounds__(256) void check_digests(const ngpu_result *__restrict__ out,
                                                     const uint8_t *__restrict__ expected,
                                                     uint64_t stride, uint32_t n,
                                                     uint64_t *__restrict__ bitmap,
                                                     unsigned long long *__restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false, unhashed = false;
  if (i < n) {
    const ngpu_result *r = out + i;
    const uint8_t *x = expected + (uint64_t)i * stride;
    unhashed = r->kind != NGPU_DIGESTED;
    uint32_t diff;
    if (VEC) {
      const uint4 a0 = reinterpret_cast<const uint4 *>(r->digest)[0];
      const uint4 a1 = reinterpret_cast<const uint4 *>(r->digest)[1];
      const uint4 b0 = reinterpret_cast<const uint4 *>(x)[0];
      const uint4 b1 = reinterpret_cast<const uint4 *>(x)[1];
      diff = (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) |
             (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w);
    } else {
      const uint32_t *a = reinterpret_cast<const uint32_t *>(r->digest);
      const uint32_t *b = reinterpret_cast<const uint32_t *>(x);
      diff = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) diff |= a[k] ^ b[k];
    }
    bad = unhashed || diff != 0;
  }
  const uint64_t word = __ballot(bad);
  // the second ballot only for a wave that holds a bad record (word is
  // wave-uniform, so every lane takes the branch together)
  uint64_t unh = 0;
  if (word) unh = __ballot(unhashed);
  // lane 0 of the wave: record i is the first of word i / 64 (256 % 64 == 0)
  if ((threadIdx.x & 63u) == 0 && i < n) {
    bitmap[i >> 6] = word;
    if (word) {
      atomicAdd(&counts[0], (unsigned long long)__popcll(word));
      if (unh) atomicAdd(&counts[1], (unsigned long long)__popcll(unh));
    }
  }
}

struct Fail {
  uint64_t order;
  ngpu_check_bad b;
};

ngpu_check_bad bad_of(const RafsV6ChunkInfo &c, uint32_t reason) {
  ngpu_check_bad b;
  memset(&b, 0, sizeof b);
  b.blob_index = c.blob_index;
  b.index = c.index;
  b.reason = reason;
  b.uncompressed_size = c.uncompressed_size;
  b.compressed_offset = c.compressed_offset;
  memcpy(b.expected, c.block_id, 32);
  return b;
}

// Each vector this feeds receives its failures in record order (the pre-pass
// over all records, the windows' inflate failures, the windows' verdicts, the
// dict probe: one vector each), so only the first `cap` of a vector can be
// among the first `cap` overall.
void keep(std::vector<Fail> &v, uint64_t cap, uint64_t order, const ngpu_check_bad &b) {
  if (v.size() < cap) v.push_back(Fail{order, b});
}

// image.blob inside a layer stream, as a blob of its own
struct SubRange {
  ngpu_read_at_fn ra;
  void *ctx;
  uint64_t base, size;
};
int64_t sub_read(void *ctx, void *buf, uint64_t len, uint64_t off) {
  const SubRange *r = (const SubRange *)ctx;
  if (off >= r->size) return -1;
  return r->ra(r->ctx, buf, std::min(len, r->size - off), r->base + off);
}

// layer: the bootstrap is a layer stream's image.boot (ngpu_check_stream); the
// stream's image.blob (own_src, a SubRange reader) is then offered as the
// layer's own blob, once the blob table is parsed, instead of `blobs`.
int check_image(ngpu_engine *e, const uint8_t *boot, uint64_t size, const ngpu_check_blob *blobs,
                uint32_t n_blobs, const LayerParts *layer, const ngpu_check_blob *own_src,
                ngpu_dict *dict, const ngpu_check_options *opt, ngpu_check_report *rep,
                ngpu_check_bad *bad, uint64_t bad_cap) {
  memset(rep, 0, sizeof *rep);
  // ---- the bootstrap's distinct chunk records ------------------------------
  uint32_t m5 = 0, m6 = 0;
  if (size >= 4) memcpy(&m5, boot, 4);
  if (size >= kRafsV6SuperBlockOffset + 4) memcpy(&m6, boot + kRafsV6SuperBlockOffset, 4);
  std::vector<RafsV6BlobInfo> btab;
  std::vector<RafsV6ChunkInfo> recs;
  uint64_t flags = 0;
  uint32_t chunk_size = 0;
  if (m6 == kRafsV6Magic) {
    Bootstrap b;
    if (int rc = parse_bootstrap(boot, size, &b)) return fail(e, rc, "check: %s", host_error());
    flags = b.flags;
    chunk_size = b.chunk_size;
    btab.swap(b.blobs);
    recs.swap(b.chunks);
  } else if (m5 == kRafsV5Magic) {
    uint32_t dg = 0;
    std::vector<uint8_t> r5, b5;
    if (int rc = parse_v5_bootstrap(boot, size, &dg, &chunk_size, &r5, &b5))
      return fail(e, rc, "check: %s", host_error());
    memcpy(&flags, boot + 16, 8);  // (parse_v5_bootstrap checked the super block's 96 bytes)
    btab.resize(b5.size() / sizeof(RafsV6BlobInfo));
    if (!b5.empty()) memcpy(btab.data(), b5.data(), btab.size() * sizeof(RafsV6BlobInfo));
    // every file's chunks, inode-table order: the distinct (blob, index) pairs
    std::unordered_set<uint64_t> seen;
    for (uint64_t i = 0; i < r5.size() / sizeof(RafsV6ChunkInfo); ++i) {
      RafsV6ChunkInfo c;
      memcpy(&c, r5.data() + i * sizeof c, sizeof c);
      if (seen.insert((uint64_t)c.blob_index << 32 | c.index).second) recs.push_back(c);
    }
  } else {
    return fail(e, NGPU_EFORMAT, "check: not a RAFS v5/v6 bootstrap");
  }
  if (flags & 0x40)  // RafsSuperFlags COMPRESSION_GZIP: the chunks live in the original gzip blob
    return fail(e, NGPU_EUNSUPP, "check: targz-ref (OCIRef) bootstrap: its blob is not chunk data");
  const uint32_t dg = (flags & 0x8) ? NGPU_DIGEST_SHA256 : NGPU_DIGEST_BLAKE3;
  if (dg != e->cfg.digester)
    return fail(e, NGPU_EINVAL, "inconsistent digester: bootstrap %s vs engine %s",
                dg ? "sha256" : "blake3", e->cfg.digester ? "sha256" : "blake3");
  if (chunk_size != e->cfg.chunk_size)
    return fail(e, NGPU_EINVAL, "inconsistent chunk size: bootstrap 0x%x vs engine 0x%x", chunk_size,
                e->cfg.chunk_size);
  ngpu_check_options o{};
  if (opt) o = *opt;
  if (!o.window_bytes) o.window_bytes = e->cfg.staging_bytes;
  if (o.window_bytes < chunk_size)
    return fail(e, NGPU_EINVAL, "check: window of %llu bytes below the chunk size 0x%x",
                (unsigned long long)o.window_bytes, chunk_size);
  o.threads = host_threads(o.threads);
  if (int rc = dict_check(e, dict)) return rc;
  if (recs.size() >= 0xFFFFFFFFull) return fail(e, NGPU_EFORMAT, "check: too many chunk records");
  rep->records = recs.size();

  std::string own_id;
  ngpu_check_blob own_blob{};
  if (layer) {  // ngpu_unpack's "own blob" rule
    const int own = own_blob_of(btab, *layer);
    n_blobs = 0;
    if (own >= 0) {
      own_id = blob_id_of(btab[own]);
      own_blob = *own_src;
      own_blob.id = own_id.c_str();
      blobs = &own_blob;
      n_blobs = 1;
    }
  }
  // bootstrap blob -> supplied blob
  std::vector<int> supplied(btab.size(), -1);
  for (size_t i = 0; i < btab.size(); ++i) {
    const std::string id = blob_id_of(btab[i]);
    for (uint32_t j = 0; j < n_blobs && supplied[i] < 0; ++j)
      if (blobs[j].id && blobs[j].ra && id == blobs[j].id) supplied[i] = (int)j;
  }

  std::vector<Fail> f_host, f_inflate, f_gpu, f_dict;
  std::vector<CheckItem> items;
  std::vector<uint64_t> dict_recs;
  for (uint64_t i = 0; i < recs.size(); ++i) {
    const RafsV6ChunkInfo &c = recs[i];
    if (c.blob_index >= btab.size())
      return fail(e, NGPU_EFORMAT, "check: chunk record %llu points at blob %u of %zu",
                  (unsigned long long)i, c.blob_index, btab.size());
    const int j = supplied[c.blob_index];
    if (j < 0) {
      if (dict) dict_recs.push_back(i);
      else ++rep->skipped;
      continue;
    }
    ++rep->checked;
    const uint64_t bsize = blobs[j].size;
    uint32_t why = 0;
    if (c.uncompressed_size == 0 || c.uncompressed_size > chunk_size ||
        c.compressed_offset > bsize || c.compressed_size > bsize - c.compressed_offset)
      why = NGPU_CHECK_RANGE;
    else if ((c.flags & 1) ? c.compressed_size > 2ull * chunk_size + 4096  // no codec grows a chunk so
                           : c.compressed_size != c.uncompressed_size)
      why = NGPU_CHECK_DECOMPRESS;
    if (why) {
      ++rep->bad;
      keep(f_host, bad_cap, i, bad_of(c, why));
      continue;
    }
    items.push_back(CheckItem{c.uncompressed_size, (uint32_t)j, i});
  }

  // ---- windows -----------------------------------------------------------
  std::vector<CheckWindow> wins;
  std::vector<uint64_t> off;
  if (!check_plan_windows(items.data(), items.size(), o.window_bytes, &wins, &off))
    return fail(e, NGPU_EINVAL, "check: a chunk does not fit the window");
  uint64_t wbytes = 0, wcount = 0;
  for (const CheckWindow &w : wins) wbytes = std::max(wbytes, w.bytes), wcount = std::max(wcount, w.count);

  // pageable targets of async copies on B.s: declared before B, whose
  // destructor synchronises the stream on every return path
  std::vector<uint8_t> dig;
  std::vector<ngpu_dict_hit> hits;
  std::vector<ngpu_result> h_res;
  DeviceGuard dg_(e->device);
  WindowBufs B(e);
  const uint64_t vwords = 2 + (wcount + 63) / 64;
  const int nbuf = wins.size() > 1 ? 2 : (int)wins.size();
  if (int rc = B.open(nbuf, wbytes, "check")) return rc;
  struct {  // what a window carries beside its bytes
    ngpu_chunk *h_ch, *d_ch;
    uint8_t *h_exp, *d_exp;
    ngpu_result *d_out;
    uint64_t *d_verdict, *h_verdict;  // [0, 2): counts, then the bitmap words
  } W[2] = {};
  for (int k = 0; k < nbuf; ++k)
    if (!B.hmalloc(&W[k].h_ch, wcount * sizeof(ngpu_chunk)) ||
        !B.dmalloc(&W[k].d_ch, wcount * sizeof(ngpu_chunk)) || !B.hmalloc(&W[k].h_exp, wcount * 32) ||
        !B.dmalloc(&W[k].d_exp, wcount * 32) || !B.dmalloc(&W[k].d_out, wcount * sizeof(ngpu_result)) ||
        !B.dmalloc(&W[k].d_verdict, vwords * 8) || !B.hmalloc(&W[k].h_verdict, vwords * 8))
      return B.no_windows(wbytes, "check");

  std::vector<uint64_t> sent[2];  // per window buffer: the items on the GPU, chunk-list order
  std::vector<uint64_t> ords;
  uint64_t unhashed = 0;
  // Window in buffer k has run: read its verdict.
  auto finish = [&](int k) -> int {
    HIP_TRY(e, hipEventSynchronize(B.done[k]));
    const uint64_t n = sent[k].size();
    const uint64_t *v = W[k].h_verdict;
    unhashed += v[1];
    if (!v[0]) return 0;
    ords.resize(v[0]);
    const uint64_t total = check_decode_bitmap(v + 2, n, ords.data(), ords.size());
    if (total != v[0])
      return fail(e, NGPU_EDEVICE, "check: bitmap holds %llu records, the counter %llu",
                  (unsigned long long)total, (unsigned long long)v[0]);
    rep->bad += total;
    if (f_gpu.size() >= bad_cap) return 0;
    h_res.resize(n);
    HIP_TRY(e, hipMemcpyAsync(h_res.data(), W[k].d_out, n * sizeof(ngpu_result), hipMemcpyDeviceToHost, B.s));
    HIP_TRY(e, hipStreamSynchronize(B.s));
    for (uint64_t q : ords) {
      const CheckItem &it = items[sent[k][q]];
      ngpu_check_bad b = bad_of(recs[it.order], NGPU_CHECK_DIGEST);
      memcpy(b.got, h_res[q].digest, 32);
      keep(f_gpu, bad_cap, it.order, b);
    }
    return 0;
  };

  for (size_t wi = 0; wi < wins.size(); ++wi) {
    const int k = (int)(wi & 1);
    if (wi >= 2)
      if (int rc = finish(k)) return rc;
    const CheckWindow &w = wins[wi];
    // fill: read + inflate the window's chunks on the pool
    std::vector<uint8_t> state(w.count, 0);  // 0 ok, 1 does not inflate, 2 reader failed
    uint8_t *h_win = (uint8_t *)B.win[k].h, *d_win = (uint8_t *)B.win[k].d;
    // every chunk is tried; the first failing one in list order is named below
    run_indexed(o.threads, w.count, [&, cbuf = std::vector<uint8_t>()](uint64_t q) mutable {
      const CheckItem &it = items[w.first + q];
      const RafsV6ChunkInfo &c = recs[it.order];
      const ngpu_check_blob &bl = blobs[it.blob];
      uint8_t *dst = h_win + off[w.first + q];
      if (!(c.flags & 1)) {
        if (!read_exact(bl.ra, bl.ctx, dst, c.compressed_size, c.compressed_offset)) state[q] = 2;
        return;
      }
      cbuf.resize(c.compressed_size);
      if (!read_exact(bl.ra, bl.ctx, cbuf.data(), c.compressed_size, c.compressed_offset))
        state[q] = 2;
      else if (decompress_chunk(btab[c.blob_index].compression_algo, cbuf.data(), c.compressed_size,
                                dst, c.uncompressed_size))
        state[q] = 1;
    });
    sent[k].clear();
    uint64_t bytes = 0;
    for (uint64_t q = 0; q < w.count; ++q) {
      const CheckItem &it = items[w.first + q];
      const RafsV6ChunkInfo &c = recs[it.order];
      if (state[q] == 2)
        return fail(e, NGPU_EIO, "check: reading chunk %u of blob %u (offset %llu, %u bytes) failed",
                    c.index, c.blob_index, (unsigned long long)c.compressed_offset, c.compressed_size);
      if (state[q] == 1) {
        ++rep->bad;
        keep(f_inflate, bad_cap, it.order, bad_of(c, NGPU_CHECK_DECOMPRESS));
        continue;
      }
      const uint64_t g = sent[k].size();
      W[k].h_ch[g] = ngpu_chunk{off[w.first + q], c.uncompressed_size, 0, 0};
      memcpy(W[k].h_exp + 32 * g, c.block_id, 32);
      sent[k].push_back(w.first + q);
      bytes += c.uncompressed_size;
    }
    const uint64_t n = sent[k].size();
    rep->bytes += bytes;
    HIP_TRY(e, hipMemcpyAsync(d_win, h_win, w.bytes, hipMemcpyHostToDevice, B.s));
    if (n) {
      HIP_TRY(e, hipMemcpyAsync(W[k].d_ch, W[k].h_ch, n * sizeof(ngpu_chunk), hipMemcpyHostToDevice, B.s));
      HIP_TRY(e, hipMemcpyAsync(W[k].d_exp, W[k].h_exp, n * 32, hipMemcpyHostToDevice, B.s));
    }
    if (int rc = ngpu_check_device(e, d_win, w.bytes, W[k].d_ch, n, W[k].d_out, W[k].d_exp, 32,
                                   W[k].d_verdict + 2, W[k].d_verdict, B.s))
      return rc;
    if (int rc = B.verdict_back(k, W[k].h_verdict, W[k].d_verdict, (2 + (n + 63) / 64) * 8)) return rc;
    e->check_windows.fetch_add(1, std::memory_order_relaxed);
  }
  for (size_t wi = wins.size() > 2 ? wins.size() - 2 : 0; wi < wins.size(); ++wi)
    if (int rc = finish((int)(wi & 1))) return rc;
  if (unhashed)
    return fail(e, NGPU_EDEVICE, "check: the digest stage left %llu record(s) unhashed",
                (unsigned long long)unhashed);

  // ---- records of blobs that are not here: the chunk dict must resolve them --
  if (!dict_recs.empty()) {
    const uint64_t n = dict_recs.size();
    uint8_t *d_dig = nullptr;
    ngpu_dict_hit *d_hits = nullptr;
    dig.resize(n * 32);
    hits.resize(n);
    for (uint64_t i = 0; i < n; ++i) memcpy(dig.data() + 32 * i, recs[dict_recs[i]].block_id, 32);
    if (!B.dmalloc(&d_dig, n * 32) || !B.dmalloc(&d_hits, n * sizeof(ngpu_dict_hit)))
      return fail(e, NGPU_ENOMEM, "check: %llu dict probes", (unsigned long long)n);
    HIP_TRY(e, hipMemcpyAsync(d_dig, dig.data(), n * 32, hipMemcpyHostToDevice, B.s));
    const ngpu_dict_hit *from = d_hits;
    if (dict->parts.empty()) {
      if (int rc = ngpu_dict_probe(dict, d_dig, 32, n, d_hits, B.s))
        return fail(e, rc, "check: dict probe failed");
      HIP_TRY(e, hipEventRecord(B.fence, B.s));
      HIP_TRY(e, hipMemcpyAsync(hits.data(), from, n * sizeof(ngpu_dict_hit), hipMemcpyDeviceToHost, B.s));
    } else {  // a node dict: through this engine's exchange (its workspace holds the buffers)
      std::lock_guard<std::mutex> g(e->mu);
      use_slot(e, B.s);
      if (int rc = ws_acquire(e, B.s)) return rc;
      ngpu_dict *replica = nullptr;
      if (int rc = node_dict_hits(e, dict, d_dig, 32, n, B.s, &from, &replica)) return rc;
      if (replica) {
        launch_dict_probe(d_dig, 32, n, replica->dev, d_hits, B.s);
        HIP_TRY(e, hipGetLastError());
        from = d_hits;
      }
      HIP_TRY(e, hipEventRecord(B.fence, B.s));
      HIP_TRY(e, hipMemcpyAsync(hits.data(), from, n * sizeof(ngpu_dict_hit), hipMemcpyDeviceToHost, B.s));
      if (int rc = ws_release(e, B.s, nullptr, false)) return rc;
    }
    HIP_TRY(e, hipStreamSynchronize(B.s));
    const uint64_t dblobs = dict->blob_table.size() / sizeof(RafsV6BlobInfo);
    for (uint64_t i = 0; i < n; ++i) {
      const RafsV6ChunkInfo &c = recs[dict_recs[i]];
      const ngpu_dict_hit &h = hits[i];
      ++rep->dict_checked;
      bool ok = h.entry != kNone && (h.usize == 0 || h.usize == c.uncompressed_size) &&
                h.index == c.index && h.uncompressed_offset == c.uncompressed_offset &&
                h.blob < dblobs;
      if (ok) {
        RafsV6BlobInfo db;
        memcpy(&db, dict->blob_table.data() + (uint64_t)h.blob * sizeof db, sizeof db);
        ok = blob_id_of(db) == blob_id_of(btab[c.blob_index]);
      }
      if (ok) continue;
      ++rep->dict_bad;
      ++rep->bad;
      keep(f_dict, bad_cap, dict_recs[i], bad_of(c, NGPU_CHECK_DICT));
    }
  }

  // ---- the first bad_cap failures, record order ---------------------------
  std::vector<Fail> all;
  all.reserve(f_host.size() + f_inflate.size() + f_gpu.size() + f_dict.size());
  for (auto *v : {&f_host, &f_inflate, &f_gpu, &f_dict}) all.insert(all.end(), v->begin(), v->end());
  std::stable_sort(all.begin(), all.end(), [](const Fail &a, const Fail &b) { return a.order < b.order; });
  for (uint64_t i = 0; i < all.size() && i < bad_cap; ++i) bad[i] = all[i].b;
  return 0;
}

}  // namespace
}  // namespace ngpu

using namespace ngpu;

extern "C" {

int ngpu_check_device(ngpu_engine *e, const void *d_data, uint64_t len, const ngpu_chunk *d_chunks,
                      uint64_t n, ngpu_result *d_out, const uint8_t *d_expected,
                      uint64_t expected_stride, uint64_t *d_bitmap, uint64_t *d_counts,
                      void *stream) {
  if (!e || !d_counts || (n && (!d_data || !d_chunks || !d_out || !d_expected || !d_bitmap)))
    return NGPU_EINVAL;
  if (n >= 0xFFFFFFFFull) return fail(e, NGPU_EINVAL, "too many chunks in one call");
  if (expected_stride < 32 || (expected_stride & 3) || ((uintptr_t)d_expected & 3))
    return fail(e, NGPU_EINVAL,
                "check: expected digests need a 4-byte aligned base and a stride >= 32 that is a "
                "multiple of 4 (stride %llu)", (unsigned long long)expected_stride);
  std::lock_guard<std::mutex> g(e->mu);
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  if (n)
    if (int rc = enqueue_digest(e, (const uint8_t *)d_data, len, d_chunks, n, d_out, s)) return rc;
  // on the caller's stream, never the null stream: a null-stream memset is not
  // ordered with a non-blocking stream's kernels ("The digest guard")
  HIP_TRY(e, hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), s));
  if (!n) return 0;
  const bool vec = (((uintptr_t)d_expected | (uintptr_t)d_out | expected_stride) & 15) == 0;
  const uint32_t grid = (uint32_t)((n + 255) / 256);
  if (vec)
    hipLaunchKernelGGL(check_digests<true>, dim3(grid), dim3(256), 0, s, d_out, d_expected,
                       expected_stride, (uint32_t)n, d_bitmap, (unsigned long long *)d_counts);
  else
    hipLaunchKernelGGL(check_digests<false>, dim3(grid), dim3(256), 0, s, d_out, d_expected,
                       expected_stride, (uint32_t)n, d_bitmap, (unsigned long long *)d_counts);
  HIP_TRY(e, hipGetLastError());
  return 0;
}

int ngpu_check_image(ngpu_engine *e, const void *bootstrap, uint64_t size,
                     const ngpu_check_blob *blobs, uint32_t n_blobs, ngpu_dict *dict,
                     const ngpu_check_options *opt, ngpu_check_report *report, ngpu_check_bad *bad,
                     uint64_t bad_cap) {
  if (!e || !bootstrap || !report || (n_blobs && !blobs) || (bad_cap && !bad)) return NGPU_EINVAL;
  return guarded_entry(e, "check", [&]() -> int {
    return check_image(e, (const uint8_t *)bootstrap, size, blobs, n_blobs, nullptr, nullptr, dict, opt,
                       report, bad, bad_cap);
  });
}

int ngpu_check_stream(ngpu_engine *e, ngpu_read_at_fn ra, void *ctx, uint64_t size, ngpu_dict *dict,
                      const ngpu_check_options *opt, ngpu_check_report *report, ngpu_check_bad *bad,
                      uint64_t bad_cap) {
  if (!e || !ra || !report || (bad_cap && !bad)) return NGPU_EINVAL;
  return guarded_entry(e, "check", [&]() -> int {
    LayerParts lp;
    if (int rc = locate_layer(ra, ctx, size, &lp)) return fail(e, rc, "check: %s", host_error());
    SubRange sr{ra, ctx, lp.data_off, lp.data_len};
    const ngpu_check_blob own_src{nullptr, sub_read, &sr, sr.size};
    return check_image(e, lp.boot.data(), lp.boot.size(), nullptr, 0, &lp, &own_src, dict, opt, report,
                       bad, bad_cap);
  });
}

}  // extern "C"
