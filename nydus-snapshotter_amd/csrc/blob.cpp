// blob.cpp — host blob stream of converter.Pack (SURVEY.md §8(f) next-3,
// §8(a) a9): what `nydus-image create --type tar-rafs --blob-inline-meta
// --features blob-toc` (pkg/converter/tool/builder.go:97-110) writes to the
// FIFO that packFromTar copies to `dest` (convert_unix.go:486-495), and the
// host readers converter.Merge needs (UnpackEntry, convert_unix.go:162-320).
//
// Stream layout (the reference reader's contract, convert_unix.go:296-300):
//   image.blob data | ustar hdr | image.boot | ustar hdr | TOC | ustar hdr
// * image.blob: the layer's NEW chunks in index order, each compressed on its
//   own (none / zstd / lz4_block) and stored raw when compression does not
//   shrink it (chunk flag bit 0 clear) — both rules as the reference v6
//   fixture shows them; compressed offsets back to back.
// * image.boot: RAFS v6 super block + extended super block, blob table at
//   4096 (256-B records) and chunk table (80-B records), as decoded from the
//   fixture.  The layer's own blob id is the sha256 of its image.blob data;
//   Merge renames it to the layer digest (see ngpu_merge).
// * rafs.blob.toc: 128-B TOCEntry records (types.go:147-163) for image.blob
//   and image.boot; calcBlobTOCDigest (convert_unix.go:541-555) = sha256 of it.
// Entry data is not padded: the reader walks back by size + 512
// (convert_unix.go:162-213).
//
// Compression stays on the host (north star): zstd / lz4 are the system
// libzstd.so.1 / liblz4.so.1, loaded with dlopen; SHA-256 is OpenSSL.
// Not byte-pinned against nydus-image (unavailable here): compressed chunk
// bytes depend on the compressor library version; the pinned properties are
// the layout rules above and the reference reader's ability to find and
// decode every entry (tests/test_blob.py).
#include <dlfcn.h>
#include <errno.h>
#include <pthread.h>
#include <signal.h>
#include <openssl/evp.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <set>
#include <unordered_map>
#include <chrono>
#include <thread>

#include "blob.hpp"
#include "rafs.hpp"

namespace ngpu {

thread_local std::string g_host_err;

int host_fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_host_err = buf;
  return code;
}

// ---- compressors ----------------------------------------------------------
struct ZInBuf {  // ZSTD_inBuffer
  const void *src;
  size_t size, pos;
};
struct ZOutBuf {  // ZSTD_outBuffer
  void *dst;
  size_t size, pos;
};

struct Codecs {
  size_t (*zstd_compress)(void *, size_t, const void *, size_t, int) = nullptr;
  size_t (*zstd_decompress)(void *, size_t, const void *, size_t) = nullptr;
  size_t (*zstd_bound)(size_t) = nullptr;
  unsigned (*zstd_is_error)(size_t) = nullptr;
  void *(*zstd_create_dstream)() = nullptr;
  size_t (*zstd_free_dstream)(void *) = nullptr;
  size_t (*zstd_decompress_stream)(void *, ZOutBuf *, ZInBuf *) = nullptr;
  int (*lz4_compress)(const char *, char *, int, int) = nullptr;
  int (*lz4_bound)(int) = nullptr;
  int (*lz4_decompress)(const char *, char *, int, int) = nullptr;
};

const Codecs &codecs() {
  static Codecs c;
  static std::once_flag once;
  std::call_once(once, [] {
    if (void *z = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL)) {
      c.zstd_compress = (decltype(c.zstd_compress))dlsym(z, "ZSTD_compress");
      c.zstd_decompress = (decltype(c.zstd_decompress))dlsym(z, "ZSTD_decompress");
      c.zstd_bound = (decltype(c.zstd_bound))dlsym(z, "ZSTD_compressBound");
      c.zstd_is_error = (decltype(c.zstd_is_error))dlsym(z, "ZSTD_isError");
      c.zstd_create_dstream = (decltype(c.zstd_create_dstream))dlsym(z, "ZSTD_createDStream");
      c.zstd_free_dstream = (decltype(c.zstd_free_dstream))dlsym(z, "ZSTD_freeDStream");
      c.zstd_decompress_stream =
          (decltype(c.zstd_decompress_stream))dlsym(z, "ZSTD_decompressStream");
    }
    if (void *l = dlopen("liblz4.so.1", RTLD_NOW | RTLD_LOCAL)) {
      c.lz4_compress = (decltype(c.lz4_compress))dlsym(l, "LZ4_compress_default");
      c.lz4_bound = (decltype(c.lz4_bound))dlsym(l, "LZ4_compressBound");
      c.lz4_decompress = (decltype(c.lz4_decompress))dlsym(l, "LZ4_decompress_safe");
    }
  });
  return c;
}

int decompress_chunk(uint32_t algo, const uint8_t *src, uint64_t csize, uint8_t *dst,
                     uint64_t usize) {
  const Codecs &c = codecs();
  if (algo == 3) {  // zstd
    if (!c.zstd_decompress) return host_fail(NGPU_EUNSUPP, "zstd unavailable (libzstd.so.1)");
    const size_t r = c.zstd_decompress(dst, usize, src, csize);
    if (c.zstd_is_error(r) || r != usize) return host_fail(NGPU_EFORMAT, "bad zstd chunk");
    return 0;
  }
  if (algo == 1) {  // lz4_block
    if (!c.lz4_decompress) return host_fail(NGPU_EUNSUPP, "lz4 unavailable (liblz4.so.1)");
    if (csize > 0x7FFFFFFF || usize > 0x7FFFFFFF) return host_fail(NGPU_EFORMAT, "bad lz4 chunk");
    const int r = c.lz4_decompress((const char *)src, (char *)dst, (int)csize, (int)usize);
    if (r < 0 || (uint64_t)r != usize) return host_fail(NGPU_EFORMAT, "bad lz4 chunk");
    return 0;
  }
  return host_fail(NGPU_EUNSUPP, "chunk compressed with unknown algorithm %u", algo);
}

namespace {

uint64_t compress_bound(uint32_t kind, uint32_t n) {
  const Codecs &c = codecs();
  if (kind == NGPU_COMPRESSOR_ZSTD) return c.zstd_bound(n);
  if (kind == NGPU_COMPRESSOR_LZ4_BLOCK) return (uint64_t)c.lz4_bound((int)n);
  return n;
}

// Compressed size, or 0 when the chunk is to be stored raw.
uint64_t compress_one(uint32_t kind, int level, const uint8_t *src, uint32_t n, uint8_t *dst,
                      uint64_t cap) {
  const Codecs &c = codecs();
  uint64_t r = 0;
  if (kind == NGPU_COMPRESSOR_ZSTD) {
    const size_t z = c.zstd_compress(dst, cap, src, n, level ? level : 1);
    r = c.zstd_is_error(z) ? 0 : z;
  } else if (kind == NGPU_COMPRESSOR_LZ4_BLOCK) {
    const int z = c.lz4_compress((const char *)src, (char *)dst, (int)n, (int)cap);
    r = z > 0 ? (uint64_t)z : 0;
  }
  return r < n ? r : 0;  // no gain: store raw (fixture: flags 0, csize == usize)
}

// nydus compress::Algorithm numbering in the blob table (fixture: lz4_block = 1)
uint32_t blob_compression_algo(uint32_t kind) {
  switch (kind) {
    case NGPU_COMPRESSOR_LZ4_BLOCK: return 1;
    case NGPU_COMPRESSOR_ZSTD: return 3;
    default: return 0;
  }
}

// RafsSuperFlags (fixture ext-SB flags 0x6 = lz4 0x2 | blake3 0x4)
uint64_t super_flags(uint32_t kind, uint32_t digester) {
  uint64_t f = digester == NGPU_DIGEST_SHA256 ? 0x8 : 0x4;
  if (kind == NGPU_COMPRESSOR_LZ4_BLOCK) f |= 0x2;
  else if (kind == NGPU_COMPRESSOR_ZSTD) f |= 0x80;
  else f |= 0x1;
  return f;
}

}  // namespace

// ---- SHA-256 (OpenSSL EVP; Sha in blob.hpp) --------------------------------

void sha256(const void *p, uint64_t n, uint8_t out[32]) {
  Sha s;
  s.update(p, n);
  s.final(out);
}

std::string hex(const uint8_t *d, int n) {
  static const char *x = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (int i = 0; i < n; ++i) {
    s[2 * i] = x[d[i] >> 4];
    s[2 * i + 1] = x[d[i] & 15];
  }
  return s;
}

namespace {

// ---- ustar headers ---------------------------------------------------------
void put_octal(char *f, int width, uint64_t v) {  // width-1 digits + NUL
  for (int i = width - 2; i >= 0; --i, v >>= 3) f[i] = (char)('0' + (v & 7));
  f[width - 1] = 0;
}

void tar_header(uint8_t h[512], const char *name, uint64_t size) {
  memset(h, 0, 512);
  char *b = (char *)h;
  strncpy(b, name, 100);
  put_octal(b + 100, 8, 0644);
  put_octal(b + 108, 8, 0);
  put_octal(b + 116, 8, 0);
  if (size < (1ull << 33)) {
    put_octal(b + 124, 12, size);
  } else {  // GNU base-256 (archive/tar parseNumeric accepts it)
    h[124] = 0x80;
    for (int i = 11; i >= 1; --i, size >>= 8) h[124 + i] = (uint8_t)size;
  }
  put_octal(b + 136, 12, 0);
  b[156] = '0';
  memcpy(b + 257, "ustar\0" "00", 8);
  memset(b + 148, ' ', 8);
  uint32_t sum = 0;
  for (int i = 0; i < 512; ++i) sum += h[i];
  put_octal(b + 148, 7, sum);
  b[155] = ' ';
}

int64_t parse_numeric(const uint8_t *f, int w) {
  if (f[0] & 0x80) {  // base-256
    uint64_t v = f[0] & 0x7f;
    for (int i = 1; i < w; ++i) v = (v << 8) | f[i];
    return (int64_t)v;
  }
  int64_t v = 0;
  int i = 0;
  while (i < w && (f[i] == ' ' || f[i] == 0)) ++i;
  for (; i < w && f[i] >= '0' && f[i] <= '7'; ++i) v = v * 8 + (f[i] - '0');
  return v;
}

// Parses one header block: name and size.  Returns false if it is not a
// valid tar header (checksum), as archive/tar's Reader.Next would fail.
bool read_header(const uint8_t h[512], std::string *name, int64_t *size) {
  uint32_t sum = 0;
  for (int i = 0; i < 512; ++i) sum += (i >= 148 && i < 156) ? ' ' : h[i];
  if ((int64_t)sum != parse_numeric(h + 148, 8)) return false;
  const char *b = (const char *)h;
  std::string nm(b, strnlen(b, 100));
  if (memcmp(b + 257, "ustar", 5) == 0 && b[345]) {  // ustar prefix
    std::string pre(b + 345, strnlen(b + 345, 155));
    nm = pre + "/" + nm;
  }
  *name = nm;
  *size = parse_numeric(h + 124, 12);
  return *size >= 0;
}

// ---- shared thread pool for per-chunk compression -------------------------
// One pool per thread count, process-wide and shared by every writer: K packs
// closing at once (containerd converting an image's layers concurrently,
// convert_unix.go:822) queue their batches on the same n threads instead of
// K pools of n (32 concurrent C1 packs used to spawn, oversubscribe and join
// 24 pools of 16 threads every round).  run() is a parallel-for any number of
// callers may be inside at once; a caller works on its own batch too.
class Pool {
 public:
  explicit Pool(unsigned n) {
    for (unsigned i = 0; i + 1 < n; ++i) th_.emplace_back([this] { loop(); });
  }
  unsigned size() const { return (unsigned)th_.size() + 1; }
  ~Pool() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : th_) t.join();
  }
  // Runs f(i) for i in [0, n) on the pool and the calling thread.
  template <typename F>
  void run(uint64_t n, F &&f) {
    if (!n) return;
    Job j;
    j.n = n;
    j.fn = f;
    {
      std::lock_guard<std::mutex> g(m_);
      q_.push_back(&j);
    }
    cv_.notify_all();
    work(j);
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [&] { return j.finished == j.n && j.users == 0; });
    for (size_t i = 0; i < q_.size(); ++i)
      if (q_[i] == &j) {
        q_.erase(q_.begin() + (long)i);
        break;
      }
  }

 private:
  struct Job {
    uint64_t n = 0;
    std::function<void(uint64_t)> fn;
    std::atomic<uint64_t> next{0};
    uint64_t finished = 0;  // items done (m_)
    unsigned users = 0;     // pool threads inside work() (m_)
  };
  // claims items of j until none is left; j stays alive while this thread is
  // counted in j.users (pool threads) or is its owner (the caller of run)
  void work(Job &j) {
    uint64_t did = 0;
    for (uint64_t i; (i = j.next.fetch_add(1)) < j.n; ++did) j.fn(i);
    std::lock_guard<std::mutex> g(m_);
    j.finished += did;
    if (j.finished == j.n) done_.notify_all();
  }
  void loop() {
    std::unique_lock<std::mutex> g(m_);
    for (;;) {
      Job *j = nullptr;
      cv_.wait(g, [&] {
        if (stop_) return true;
        for (Job *x : q_)  // the oldest batch with items left
          if (x->next.load() < x->n) {
            j = x;
            return true;
          }
        return false;
      });
      if (stop_) return;
      ++j->users;
      g.unlock();
      work(*j);
      g.lock();
      if (--j->users == 0) done_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::vector<Job *> q_;  // batches with callers inside run()
  bool stop_ = false;
  std::mutex m_;
  std::condition_variable cv_, done_;
};

// A batch buffer of the blob stream, grown by new[] -- no zero fill (a 64 MiB
// std::vector resize is ~10 ms of memset on a writer's first batches; every
// byte is written before the sink reads it).
struct Batch {
  std::unique_ptr<uint8_t[]> p;
  uint64_t cap = 0, n = 0;
  // non-empty: the batch's stream bytes are these pieces, in order (into p
  // or into caller memory that outlives the writer's finish), not p[0, n)
  std::vector<std::pair<const uint8_t *, uint64_t>> seg;
  void resize(uint64_t k) {
    if (k > cap) {
      p.reset(new uint8_t[k]);
      cap = k;
    }
    n = k;
  }
  uint8_t *data() { return p.get(); }
  uint64_t size() const { return n; }
  uint8_t &operator[](uint64_t i) { return p[i]; }
};

// A writer lives for one Pack; the compression pools are shared and its
// batch / scratch buffers stay for the next writers (joining a 16-thread pool
// and unmapping three 64 MiB buffers were ~20 ms of every early-emission
// Pack's close, the next writer's first batches paid the page faults again,
// and 32 concurrent packs overflowed an 8-buffer cache every round).  Buffers
// are kept up to kCacheBytes.  Process-wide, never destroyed (no exit-time
// teardown of idle threads).
struct WriterCache {
  // (a batch buffer holds <= 64 MiB of input at compressBound: a bit over)
  static constexpr uint64_t kBufMax = 80ull << 20, kCacheBytes = 2ull << 30;
  std::mutex m;
  std::vector<std::unique_ptr<Pool>> pools;
  std::vector<Batch> bufs;
  uint64_t cached = 0;  // bytes in bufs
  static WriterCache &get() {
    static WriterCache *c = new WriterCache;
    return *c;
  }
  // the process-wide pool of n threads (created on first use, never destroyed)
  Pool *pool(unsigned n) {
    std::lock_guard<std::mutex> g(m);
    for (auto &p : pools)
      if (p->size() == n) return p.get();
    pools.emplace_back(new Pool(n));
    return pools.back().get();
  }
  bool take_buf(Batch *b) {
    std::lock_guard<std::mutex> g(m);
    if (bufs.empty()) return false;
    *b = std::move(bufs.back());
    bufs.pop_back();
    cached -= b->cap;
    return true;
  }
  void put_buf(Batch &&b) {
    if (!b.p || b.cap > kBufMax) return;
    std::lock_guard<std::mutex> g(m);
    if (cached + b.cap > kCacheBytes) return;
    cached += b.cap;
    bufs.push_back(std::move(b));
  }
};

}  // namespace

const char *host_error() { return g_host_err.c_str(); }

std::string blob_id_of(const RafsV6BlobInfo &b) {
  return std::string(b.blob_id, strnlen(b.blob_id, sizeof b.blob_id));
}

int parse_bootstrap(const uint8_t *p, uint64_t n, Bootstrap *out, bool with_chunks) {
  if (n < kRafsV6ExtSuperBlockOffset + 64) return host_fail(NGPU_EFORMAT, "bootstrap too small");
  uint32_t magic;
  memcpy(&magic, p + kRafsV6SuperBlockOffset, 4);
  if (magic != kRafsV6Magic) return host_fail(NGPU_EFORMAT, "not a RAFS v6 bootstrap");
  const uint8_t *x = p + kRafsV6ExtSuperBlockOffset;
  uint64_t bto, cto, cts;
  uint32_t bts;
  memcpy(&out->flags, x, 8);
  memcpy(&bto, x + 8, 8);
  memcpy(&bts, x + 16, 4);
  memcpy(&out->chunk_size, x + 20, 4);
  memcpy(&cto, x + 24, 8);  // RafsV6ChunkInfoOffset = 1024+128+24 (layout.go:27)
  memcpy(&cts, x + 32, 8);
  if (bts % sizeof(RafsV6BlobInfo) || cts % sizeof(RafsV6ChunkInfo) || bto > n ||
      bts > n - bto || cto > n || cts > n - cto)
    return host_fail(NGPU_EFORMAT, "bad blob/chunk table bounds");
  out->blobs.resize(bts / sizeof(RafsV6BlobInfo));
  if (bts) memcpy(out->blobs.data(), p + bto, bts);
  if (!with_chunks) return 0;
  out->chunks.resize(cts / sizeof(RafsV6ChunkInfo));
  if (cts) memcpy(out->chunks.data(), p + cto, cts);
  return 0;
}

namespace {
template <typename T>
T rd_le(const uint8_t *p) {
  T v;
  memcpy(&v, p, sizeof v);
  return v;
}
}  // namespace

// A RAFS v5 chunk-dict bootstrap (FsVersion "5" with ChunkDictPath).  v5
// keeps no chunk table: each regular file's RafsV5ChunkInfo records (80 B,
// the same fields as the v6 chunk info) follow its inode, so the dict is
// every file's chunks in inode-table order (HashChunkDict keeps the first
// insertion of a digest).  Layout restated from [nydus v2.3.0]
// rafs/src/metadata/layout/v5.rs (VERIFY), as decoded and checked on the
// reference fixture pkg/filesystem/testdata/v5-bootstrap-file-size-736032
// (tests/rafs_fixtures.py):
//   super block (8 KiB): magic u32, fs_version u32, sb_size u32, block_size
//     u32, flags u64, inodes_count u64, inode_table_offset u64,
//     prefetch_table_offset u64, blob_table_offset u64, inode_table_entries
//     u32, prefetch_table_entries u32, blob_table_size u32,
//     extended_blob_table_entries u32, extended_blob_table_offset u64;
//   inode table: u32 per entry = inode offset >> 3 (0 = unused);
//   inode (128 B): ... mode u32 @60, size u64 @64, flags u64 @80 (SYMLINK 1,
//     XATTR 4), child_count u32 @96, name_size u16 @100, symlink_size u16
//     @102; then the name and symlink (8-B padded), the xattr table (u64 size
//     + data, 8-B padded) when XATTR, then child_count chunk infos;
//   blob table: {readahead offset u32, size u32, blob id up to NUL}, 8-B
//     padded; extended blob table: 64-B entries {chunk_count u32, reserved
//     u32, uncompressed_size u64, compressed_size u64, ...}.
// Its blobs become 256-B v6 blob records (id, chunk size / count, sizes,
// digester) for the layer bootstraps the blob writer emits (a v5 Pack writes
// a v6-format image.boot).
int parse_v5_bootstrap(const uint8_t *p, uint64_t n, uint32_t *digester, uint32_t *chunk_size,
                       std::vector<uint8_t> *recs_out, std::vector<uint8_t> *blobs_out) {
  if (n < 96) return host_fail(NGPU_EFORMAT, "truncated RAFS v5 super block");
  const uint32_t bs = rd_le<uint32_t>(p + 12);
  const uint64_t flags = rd_le<uint64_t>(p + 16);
  const uint64_t ito = rd_le<uint64_t>(p + 32), bto = rd_le<uint64_t>(p + 48);
  const uint32_t ient = rd_le<uint32_t>(p + 56), btsz = rd_le<uint32_t>(p + 64);
  const uint32_t xbent = rd_le<uint32_t>(p + 68);
  const uint64_t xbto = rd_le<uint64_t>(p + 72);
  const uint32_t dg = (flags & 0x8) ? NGPU_DIGEST_SHA256 : NGPU_DIGEST_BLAKE3;
  *digester = dg;
  *chunk_size = bs;
  if (ito > n || (uint64_t)ient * 4 > n - ito || bto > n || btsz > n - bto || xbto > n ||
      (uint64_t)xbent * 64 > n - xbto)
    return host_fail(NGPU_EFORMAT, "bad RAFS v5 table bounds");
  // blob ids
  std::vector<std::string> ids;
  for (uint64_t q = bto, end = bto + btsz; q + 8 < end;) {
    const uint8_t *z = (const uint8_t *)memchr(p + q + 8, 0, end - q - 8);
    const uint64_t e2 = z ? (uint64_t)(z - p) : end;
    ids.emplace_back((const char *)p + q + 8, e2 - q - 8);
    q = (e2 + 1 + 7) / 8 * 8;
  }
  // chunk infos, file by file in inode-table order
  std::vector<uint8_t> &recs = *recs_out;
  recs.clear();
  for (uint32_t i = 0; i < ient; ++i) {
    const uint32_t o = rd_le<uint32_t>(p + ito + 4ull * i);
    if (!o) continue;
    const uint64_t off = (uint64_t)o << 3;
    if (off > n || n - off < 128)
      return host_fail(NGPU_EFORMAT, "inode %u out of bounds", i);
    const uint8_t *in = p + off;
    const uint32_t mode = rd_le<uint32_t>(in + 60);
    const uint64_t size = rd_le<uint64_t>(in + 64), ifl = rd_le<uint64_t>(in + 80);
    const uint32_t cc = rd_le<uint32_t>(in + 96);
    const uint16_t nsz = rd_le<uint16_t>(in + 100), slsz = rd_le<uint16_t>(in + 102);
    uint64_t q = off + 128 + (nsz + 7) / 8 * 8;
    if (ifl & 0x1) q += (slsz + 7) / 8 * 8;
    if (ifl & 0x4) {
      if (q > n || n - q < 8)
        return host_fail(NGPU_EFORMAT, "xattrs of inode %u out of bounds", i);
      const uint64_t xs = rd_le<uint64_t>(p + q);
      if (xs > n) return host_fail(NGPU_EFORMAT, "bad xattr size");
      q += 8 + (xs + 7) / 8 * 8;
    }
    if ((mode & 0170000) != 0100000 || size == 0) continue;  // regular files with data
    if (q > n || (uint64_t)cc * 80 > n - q)
      return host_fail(NGPU_EFORMAT, "chunks of inode %u out of bounds", i);
    for (uint32_t k = 0; k < cc; ++k) {
      if (rd_le<uint32_t>(p + q + 80ull * k + 32) >= ids.size())
        return host_fail(NGPU_EFORMAT, "chunk blob index out of range");
    }
    recs.insert(recs.end(), p + q, p + q + 80ull * cc);
  }
  // blobs as v6 blob records
  blobs_out->assign(ids.size() * sizeof(RafsV6BlobInfo), 0);
  for (size_t i = 0; i < ids.size(); ++i) {
    RafsV6BlobInfo bi{};
    memcpy(bi.blob_id, ids[i].data(), std::min<size_t>(ids[i].size(), sizeof bi.blob_id));
    bi.blob_index = (uint32_t)i;
    bi.chunk_size = bs;
    bi.digest_algo = dg == NGPU_DIGEST_SHA256 ? 1 : 0;
    // RafsSuperFlags compressor bits -> compress::Algorithm (lz4_block 0x2 -> 1, as
    // the v6 fixture's flags and blob record pair them; zstd 0x80 -> 3)
    bi.compression_algo = (flags & 0x2) ? 1 : (flags & 0x80) ? 3 : 0;
    if (i < xbent) {
      const uint8_t *x = p + xbto + 64 * i;
      bi.chunk_count = rd_le<uint32_t>(x);
      bi.uncompressed_size = rd_le<uint64_t>(x + 8);
      bi.compressed_size = rd_le<uint64_t>(x + 16);
    }
    memcpy(blobs_out->data() + i * sizeof bi, &bi, sizeof bi);
  }
  return 0;
}


std::vector<uint8_t> write_bootstrap(const Bootstrap &b) {
  const uint64_t bts = b.blobs.size() * sizeof(RafsV6BlobInfo);
  const uint64_t cto = kBlobTableOffset + (bts + 4095) / 4096 * 4096;
  const uint64_t cts = b.chunks.size() * sizeof(RafsV6ChunkInfo);
  std::vector<uint8_t> v(cto + cts, 0);
  memcpy(&v[kRafsV6SuperBlockOffset], &kRafsV6Magic, 4);
  uint8_t *x = &v[kRafsV6ExtSuperBlockOffset];
  const uint64_t bto = bts ? kBlobTableOffset : 0;
  const uint32_t bts32 = (uint32_t)bts;
  memcpy(x, &b.flags, 8);
  memcpy(x + 8, &bto, 8);
  memcpy(x + 16, &bts32, 4);
  memcpy(x + 20, &b.chunk_size, 4);
  memcpy(x + 24, &cto, 8);
  memcpy(x + 32, &cts, 8);
  if (bts) memcpy(&v[kBlobTableOffset], b.blobs.data(), bts);
  if (cts) memcpy(&v[cto], b.chunks.data(), cts);
  return v;
}

// ---- BlobWriter --------------------------------------------------------------
struct BlobWriter::Impl {
  ngpu_blob_options opt;
  ngpu_write_fn w;
  void *ctx;
  std::vector<RafsV6BlobInfo> dict_blobs;
  const DictPlace *dict_place = nullptr;
  uint64_t n_place = 0;
  const volatile int32_t *cancel = nullptr;
  const ZranRef *zref = nullptr;  // OCIRef: the own blob is the original gzip blob
  Pool *pool = nullptr;  // shared (WriterCache)
  Sha blob_sha;      // image.blob data
  Sha stream_sha;    // whole stream (continued from blob_sha)
  uint64_t written = 0;
  std::vector<uint32_t> csize;  // per NEW chunk (index order)
  std::vector<uint8_t> cflag;
  uint64_t compressed_chunks = 0;
  uint64_t batches_added = 0;  // batches submitted by add()
  // per batch: each chunk's bound-sized slot of the batch buffer (slot_off)
  std::vector<uint64_t> slot_off;
  std::vector<uint64_t> clen;
  int rc = 0;
  // Sink thread: SHA-256 + dest write of finished batches, so the single
  // sequential hash overlaps the next batch's compression / copy and the
  // GPU gather of the next window (at most kDepth batches in flight).
  static constexpr size_t kDepth = 2;

  std::thread sink;
  std::mutex qm;
  std::condition_variable qcv;
  std::deque<Batch> q, free_bufs;
  bool busy = false, stop = false;
  int sink_rc = 0;
  std::string sink_err;

  int emit(const void *p, uint64_t n) {
    if (!n) return 0;
    if (w && w(ctx, p, n) != 0) return host_fail(NGPU_EIO, "pack: dest write failed");
    written += n;
    return 0;
  }
  // NGPU_SINK_STATS=1: the sink's time split, printed to stderr when the
  // writer goes (diagnostic of the stream's single-thread bound)
  double t_wait = 0, t_sha = 0, t_emit = 0, t_first = -1, t_last = 0;
  uint64_t n_batches = 0;
  const std::chrono::steady_clock::time_point t_born = std::chrono::steady_clock::now();
  void sink_loop() {
    using clk = std::chrono::steady_clock;
    std::unique_lock<std::mutex> g(qm);
    for (;;) {
      const auto t0 = clk::now();
      qcv.wait(g, [&] { return stop || !q.empty(); });
      const auto t1 = clk::now();
      if (n_batches) t_wait += std::chrono::duration<double>(t1 - t0).count();
      else t_first = std::chrono::duration<double>(t1 - t_born).count();
      if (q.empty()) return;
      Batch b = std::move(q.front());
      q.pop_front();
      busy = true;
      const bool failed = sink_rc != 0;
      g.unlock();
      int r = 0;
      if (!failed) {
        if (b.seg.empty()) {
          blob_sha.update(b.data(), b.size());
        } else {
          for (const auto &sg : b.seg) blob_sha.update(sg.first, sg.second);
        }
        const auto t2 = clk::now();
        if (b.seg.empty()) {
          r = emit(b.data(), b.size());
        } else {
          for (const auto &sg : b.seg)
            if ((r = emit(sg.first, sg.second))) break;
        }
        t_sha += std::chrono::duration<double>(t2 - t1).count();
        t_emit += std::chrono::duration<double>(clk::now() - t2).count();
      }
      ++n_batches;
      t_last = std::chrono::duration<double>(clk::now() - t_born).count();
      g.lock();
      if (r && !sink_rc) {
        sink_rc = r;
        sink_err = host_error();
      }
      busy = false;
      free_bufs.push_back(std::move(b));
      qcv.notify_all();
    }
  }
  Batch take_buffer() {
    std::unique_lock<std::mutex> g(qm);
    qcv.wait(g, [&] { return q.size() < kDepth; });
    Batch b;
    if (free_bufs.empty()) {
      (void)WriterCache::get().take_buf(&b);  // one an earlier writer left
      return b;
    }
    b = std::move(free_bufs.front());
    free_bufs.pop_front();
    return b;
  }
  int submit(Batch &&b) {
    std::lock_guard<std::mutex> g(qm);
    if (sink_rc) return host_fail(sink_rc, "%s", sink_err.c_str());
    q.push_back(std::move(b));
    qcv.notify_all();
    return 0;
  }
  int drain() {  // wait for the sink; its error becomes this thread's
    std::unique_lock<std::mutex> g(qm);
    qcv.wait(g, [&] { return q.empty() && !busy; });
    if (sink_rc) return host_fail(sink_rc, "%s", sink_err.c_str());
    return 0;
  }
  ~Impl() {
    {
      std::lock_guard<std::mutex> g(qm);
      stop = true;
    }
    qcv.notify_all();
    if (sink.joinable()) sink.join();
    WriterCache &wc = WriterCache::get();
    for (Batch &b : free_bufs) wc.put_buf(std::move(b));
    for (Batch &b : q) wc.put_buf(std::move(b));
    const char *v = getenv("NGPU_SINK_STATS");
    if (v && *v == '1')
      fprintf(stderr, "{\"sink_batches\": %llu, \"sink_wait_s\": %.4f, \"sink_sha_s\": %.4f, "
              "\"sink_emit_s\": %.4f, \"first_batch_at_s\": %.4f, \"last_batch_done_at_s\": %.4f, "
              "\"writer_gone_at_s\": %.4f, \"bytes\": %llu}\n", (unsigned long long)n_batches, t_wait,
              t_sha, t_emit, t_first, t_last,
              std::chrono::duration<double>(std::chrono::steady_clock::now() - t_born).count(),
              (unsigned long long)written);
  }
};

BlobWriter::BlobWriter(const ngpu_blob_options &opt, ngpu_write_fn w, void *ctx,
                       std::vector<RafsV6BlobInfo> dict_blobs, const DictPlace *dict_place,
                       uint64_t n_place)
    : im_(new Impl) {
  im_->opt = opt;
  if (!im_->opt.compressor) im_->opt.compressor = NGPU_COMPRESSOR_ZSTD;
  im_->w = w;
  im_->ctx = ctx;
  im_->dict_blobs = std::move(dict_blobs);
  im_->dict_place = dict_place;
  im_->n_place = dict_place ? n_place : 0;
}

void BlobWriter::set_cancel(const volatile int32_t *flag) { im_->cancel = flag; }
void BlobWriter::set_zran(const ZranRef *z) { im_->zref = z; }

BlobWriter::~BlobWriter() = default;

int BlobWriter::init() {
  const uint32_t k = im_->opt.compressor;
  const Codecs &c = codecs();
  if (k == NGPU_COMPRESSOR_ZSTD && !(c.zstd_compress && c.zstd_bound && c.zstd_is_error))
    return host_fail(NGPU_EUNSUPP, "zstd compressor unavailable (libzstd.so.1)");
  if (k == NGPU_COMPRESSOR_LZ4_BLOCK && !(c.lz4_compress && c.lz4_bound))
    return host_fail(NGPU_EUNSUPP, "lz4_block compressor unavailable (liblz4.so.1)");
  if (k != NGPU_COMPRESSOR_NONE && k != NGPU_COMPRESSOR_ZSTD && k != NGPU_COMPRESSOR_LZ4_BLOCK)
    return host_fail(NGPU_EINVAL, "unsupported compressor 0x%x", k);
  unsigned t = im_->opt.threads;
  if (!t) {
    const unsigned hw = std::thread::hardware_concurrency();
    t = hw ? std::min(16u, hw) : 4u;
  }
  im_->pool = WriterCache::get().pool(t);
  Impl *m = im_.get();
  m->sink = std::thread([m] { m->sink_loop(); });
  return 0;
}

int BlobWriter::add(const uint8_t *const *src, const uint32_t *len, uint64_t k, bool src_stable) {
  Impl &m = *im_;
  if (m.rc) return m.rc;
  const uint32_t kind = m.opt.compressor;
  // batches of <= 64 MiB of input keep the buffers bounded (smaller first ones, below)
  uint64_t a = 0;
  while (a < k) {
    if (m.cancel && __atomic_load_n(m.cancel, __ATOMIC_RELAXED))
      return m.rc = host_fail(NGPU_ECANCELED, "pack: cancelled");
    uint64_t b = a, bytes = 0;
    // batches grow 4, 8, 16, 32, then 64 MiB of input: the sink starts hashing
    // the first while the next compresses (a 10 MB layer used to compress all
    // of it, then hash all of it), and big layers still run in large batches
    const uint64_t lim = std::min<uint64_t>(64ull << 20, 4ull << (20 + std::min<uint64_t>(m.batches_added, 4)));
    while (b < k && (b == a || bytes + len[b] <= lim)) bytes += len[b++];
    ++m.batches_added;
    const uint64_t nb = b - a;
    Batch out = m.take_buffer();
    out.seg.clear();
    if (kind == NGPU_COMPRESSOR_NONE && src_stable) {  // the caller's bytes are the stream
      out.resize(0);
      for (uint64_t i = 0; i < nb; ++i) {
        out.seg.emplace_back(src[a + i], len[a + i]);
        m.csize.push_back(len[a + i]);
        m.cflag.push_back(0);
      }
    } else if (kind == NGPU_COMPRESSOR_NONE) {
      out.resize(bytes);
      m.slot_off.resize(nb + 1);
      m.slot_off[0] = 0;
      for (uint64_t i = 0; i < nb; ++i) m.slot_off[i + 1] = m.slot_off[i] + len[a + i];
      m.pool->run(nb, [&](uint64_t i) { memcpy(&out[m.slot_off[i]], src[a + i], len[a + i]); });
      for (uint64_t i = 0; i < nb; ++i) {
        m.csize.push_back(len[a + i]);
        m.cflag.push_back(0);
      }
    } else {
      m.slot_off.resize(nb + 1);
      m.slot_off[0] = 0;
      for (uint64_t i = 0; i < nb; ++i)
        m.slot_off[i + 1] = m.slot_off[i] + compress_bound(kind, len[a + i]);
      // every chunk compresses into its own bound-sized slot of the batch
      // buffer, and the batch is the list of those pieces: no compaction
      // copy.  A chunk that does not shrink is stored raw: a piece of the
      // caller's memory when it outlives the writer (src_stable: the pinned
      // staging slot of a one-slot layer), else copied into its slot (the
      // blob windows' landing buffers are reused by the next window).
      out.resize(m.slot_off[nb]);
      m.clen.assign(nb, 0);
      m.pool->run(nb, [&](uint64_t i) {
        m.clen[i] = compress_one(kind, m.opt.level, src[a + i], len[a + i], &out[m.slot_off[i]],
                                 m.slot_off[i + 1] - m.slot_off[i]);
        if (!m.clen[i] && !src_stable) memcpy(&out[m.slot_off[i]], src[a + i], len[a + i]);
      });
      for (uint64_t i = 0; i < nb; ++i) {
        const bool z = m.clen[i] != 0;
        const uint64_t c = z ? m.clen[i] : len[a + i];
        out.seg.emplace_back(z || !src_stable ? &out[m.slot_off[i]] : src[a + i], c);
        m.csize.push_back((uint32_t)c);
        m.cflag.push_back(z ? 1 : 0);
        m.compressed_chunks += z;
      }
    }
    if ((m.rc = m.submit(std::move(out)))) return m.rc;
    a = b;
  }
  return 0;
}

int BlobWriter::finish(const ngpu_chunk *chunks, const ngpu_result *res, uint64_t n,
                       const ngpu_layer_stats &st, const std::vector<TarEntry> &entries,
                       ngpu_blob_info *info) {
  Impl &m = *im_;
  if (m.rc) return m.rc;
  if ((m.rc = m.drain())) return m.rc;
  const uint32_t fs_version = m.opt.fs_version ? m.opt.fs_version : 6;
  if (fs_version != 5 && fs_version != 6)
    return m.rc = host_fail(NGPU_EINVAL, "pack: FsVersion %u", fs_version);
  const uint32_t kind = m.opt.compressor;
  const uint64_t blob_bytes = m.written;
  // image.blob digest; the stream digest continues from the same state
  uint8_t blob_dig[32], boot_dig[32], toc_dig[32], stream_dig[32];
  m.stream_sha.copy_from(m.blob_sha);
  m.blob_sha.final(blob_dig);

  // chunk table: NEW chunks in index order with their compressed placement
  Bootstrap b;
  b.flags = super_flags(kind, m.opt.digester);
  b.chunk_size = m.opt.chunk_size;
  const ZranRef *zr = m.zref;
  if (zr) b.flags = (b.flags & ~0x83ull) | 0x40;  // RafsSuperFlags COMPRESSION_GZIP (VERIFY)
  const uint64_t bodies = zr ? zr->coff.size() : m.csize.size();
  uint64_t k = 0, coff = 0, uend = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const ngpu_result &r = res[i];
    if (r.kind != NGPU_NEW) continue;
    if (r.index != k || k >= bodies)
      return host_fail(NGPU_EINVAL, "pack: NEW chunk %llu out of index order",
                       (unsigned long long)i);
    RafsV6ChunkInfo c;
    memset(&c, 0, sizeof c);
    memcpy(c.block_id, r.digest, 32);
    c.blob_index = r.blob_index;
    if (zr) {  // targz-ref: the chunk's deflate range in the original gzip blob
      // (an oversized range is refused, never truncated: the
      // chunk-info v2 entry holds compressed size - 1 in 24 bits and the
      // offset in 40)
      if (zr->csize[k] == 0 || zr->csize[k] > (1ull << 24) || zr->coff[k] >= (1ull << 40))
        return host_fail(NGPU_EFORMAT,
                         "targz-ref: chunk %llu's deflate range (%llu B at %llu) does not fit the "
                         "blob.meta chunk entry (24-bit size, 40-bit offset)",
                         (unsigned long long)i, (unsigned long long)zr->csize[k],
                         (unsigned long long)zr->coff[k]);
      c.flags = 1;  // compressed (gzip, through its checkpoint)
      c.compressed_size = (uint32_t)zr->csize[k];
      c.compressed_offset = zr->coff[k];
    } else {
      c.flags = m.cflag[k];
      c.compressed_size = m.csize[k];
      c.compressed_offset = coff;
      coff += m.csize[k];
    }
    c.uncompressed_size = chunks[i].length;
    c.uncompressed_offset = r.uncompressed_offset;
    c.file_offset = chunks[i].file_offset;
    c.index = r.index;
    b.chunks.push_back(c);
    uend = std::max<uint64_t>(uend, r.uncompressed_offset + chunks[i].length);
    ++k;
  }
  if (k != bodies) return host_fail(NGPU_EINVAL, "pack: %llu chunk bodies for %llu NEW chunks",
                                    (unsigned long long)bodies, (unsigned long long)k);
  // every chunk's record, for the inode tree: a NEW or INTRA chunk points at
  // the NEW record of its index, a DICT chunk at the dict's copy (below)
  RafsLayerInfo li;
  li.fs_version = fs_version;
  li.chunk_size = m.opt.chunk_size;
  li.digester = m.opt.digester;
  li.flags = b.flags;
  // NULL or "" -> "/" (nydus_gpu.h ngpu_blob_options; builder.go:125-127): an
  // empty string from a binding must not drop the prefetch table
  if (m.opt.prefetch_patterns && *m.opt.prefetch_patterns) li.prefetch = m.opt.prefetch_patterns;
  li.refs.resize(n);
  li.file_of.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    const ngpu_result &r = res[i];
    li.file_of[i] = chunks[i].file_index;
    if (r.kind == NGPU_NEW || r.kind == NGPU_INTRA) {
      if (r.index >= k) return host_fail(NGPU_EINVAL, "pack: chunk %llu index out of range",
                                         (unsigned long long)i);
      li.refs[i] = b.chunks[r.index];
    } else if (r.kind != NGPU_DICT) {
      return host_fail(NGPU_EINVAL, "pack: chunk %llu has no dedup decision (kind %u)",
                       (unsigned long long)i, r.kind);
    }
    li.refs[i].file_offset = chunks[i].file_offset;
  }
  // Chunk-dict chunks the layer reuses: one record per distinct (digest, real
  // blob), a copy of the dict's record ([nydus v2.3.0] deduplicate_chunk:
  // chunk.copy_from(cached_chunk) + set_file_offset + the real blob index;
  // the v6 chunk table holds every distinct chunk a node references, keyed
  // by digest and blob index -- VERIFY), first occurrence in stream order.
  uint64_t ndict = 0;
  {
    std::vector<std::pair<std::array<uint8_t, 32>, uint32_t>> seen;
    std::vector<uint64_t> order;
    for (uint64_t i = 0; i < n; ++i)
      if (res[i].kind == NGPU_DICT) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
      const int c = memcmp(res[x].digest, res[y].digest, 32);
      if (c) return c < 0;
      if (res[x].blob_index != res[y].blob_index) return res[x].blob_index < res[y].blob_index;
      return x < y;
    });
    std::vector<uint64_t> firsts;
    for (size_t j = 0; j < order.size(); ++j) {
      const uint64_t i = order[j];
      if (j && memcmp(res[order[j - 1]].digest, res[i].digest, 32) == 0 &&
          res[order[j - 1]].blob_index == res[i].blob_index)
        continue;
      firsts.push_back(i);
    }
    std::sort(firsts.begin(), firsts.end());
    auto dict_record = [&](uint64_t i) {
      const ngpu_result &r = res[i];
      RafsV6ChunkInfo c;
      memset(&c, 0, sizeof c);
      memcpy(c.block_id, r.digest, 32);
      c.blob_index = r.blob_index;
      c.uncompressed_size = chunks[i].length;
      if (r.ref < m.n_place) {
        const DictPlace &pl = m.dict_place[r.ref];
        c.flags = pl.flags;
        c.compressed_size = pl.compressed_size;
        c.compressed_offset = pl.compressed_offset;
      } else {  // dict given without its chunk records: stored raw
        c.compressed_size = chunks[i].length;
      }
      c.uncompressed_offset = r.uncompressed_offset;
      c.file_offset = chunks[i].file_offset;
      c.index = r.index;
      return c;
    };
    for (uint64_t i : firsts) {
      b.chunks.push_back(dict_record(i));
      ++ndict;
    }
    for (uint64_t i : order) li.refs[i] = dict_record(i);
  }
  // blob table in real-index (first-hit) order
  b.blobs.assign(st.blobs, RafsV6BlobInfo{});
  std::vector<bool> set(st.blobs, false);
  if (st.own_blob_index != 0xFFFFFFFFu) {
    if (st.own_blob_index >= st.blobs) return host_fail(NGPU_EINVAL, "pack: bad own blob index");
    RafsV6BlobInfo &o = b.blobs[st.own_blob_index];
    const std::string id = hex(zr ? zr->digest : blob_dig, 32);  // targz-ref: the gzip blob's digest
    memcpy(o.blob_id, id.data(), 64);
    o.chunk_size = m.opt.chunk_size;
    o.chunk_count = (uint32_t)k;
    o.compression_algo = zr ? 2 : blob_compression_algo(kind);  // compress::Algorithm GZip (VERIFY)
    o.digest_algo = m.opt.digester == NGPU_DIGEST_SHA256 ? 1 : 0;
    o.features = 1;
    o.compressed_size = zr ? zr->gz_size : coff;
    o.uncompressed_size = (uend + 4095) / 4096 * 4096;
    set[st.own_blob_index] = true;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const ngpu_result &r = res[i];
    if (r.kind != NGPU_DICT) continue;
    if (r.blob_index >= st.blobs) return host_fail(NGPU_EINVAL, "pack: bad dict blob index");
    if (set[r.blob_index]) continue;
    RafsV6BlobInfo &d = b.blobs[r.blob_index];
    if (r.dict_blob < m.dict_blobs.size()) {
      d = m.dict_blobs[r.dict_blob];
    } else {  // dict given as arrays without a blob table: a stable placeholder id
      char id[65];
      snprintf(id, sizeof id, "%064x", r.dict_blob);
      memcpy(d.blob_id, id, 64);
      d.chunk_size = m.opt.chunk_size;
    }
    set[r.blob_index] = true;
  }
  for (uint32_t i = 0; i < st.blobs; ++i) {
    if (!set[i]) return host_fail(NGPU_EINVAL, "pack: blob %u never referenced", i);
    b.blobs[i].blob_index = i;
  }

  // tail (stream offsets from blob_bytes on):
  //   hdr(image.blob) | blob.meta: ci array + ci header | hdr(blob.meta) |
  //   blob.digest | hdr(blob.digest) | image.boot | hdr(image.boot) | TOC | hdr(toc)
  std::vector<uint8_t> tail;
  std::vector<TocEntry> toc;
  auto put = [&](const void *p, uint64_t len) {
    tail.insert(tail.end(), (const uint8_t *)p, (const uint8_t *)p + len);
  };
  auto hdr = [&](const char *name, uint64_t size) {
    uint8_t h[512];
    tar_header(h, name, size);
    put(h, 512);
  };
  auto toc_add = [&](const char *name, uint32_t flags, const uint8_t dig[32], uint64_t off,
                     uint64_t csize, uint64_t usize) {
    TocEntry e;
    memset(&e, 0, sizeof e);
    e.flags = flags;
    memcpy(e.name, name, std::min(strlen(name), sizeof e.name));  // NUL-padded, 16 chars max
    memcpy(e.uncompressed_digest, dig, 32);
    e.compressed_offset = off;
    e.compressed_size = csize;
    e.uncompressed_size = usize;
    toc.push_back(e);
  };
  if (!zr) {  // targz-ref: the data stays in the original gzip blob, no image.blob
    toc_add("image.blob", NGPU_COMPRESSOR_NONE, blob_dig, 0, blob_bytes, blob_bytes);
    hdr("image.blob", blob_bytes);
  }
  // blob.meta / blob.meta.header / blob.digest (convert_unix.go:47-48 names the
  // first two; `--blob-inline-meta --features blob-toc`, builder.go:97-110,
  // makes nydus-image write all three for a blob with chunks).  Restated from
  // [nydus v2.3.0] builder/src/core/blob.rs Blob::dump_meta_data and
  // storage/src/meta (VERIFY): the chunk-info array (BlobChunkInfoV2, 24 B per
  // chunk of the layer's own blob, index order), compressed like the chunks
  // when that shrinks it, then the 4 KiB BlobCompressionContextHeader, under
  // one tar entry; the TOC has an entry for each part.  The V2 entry keeps the
  // uncompressed offset in 4 KiB units, so a blob whose offsets are not 4 KiB
  // aligned (RAFS v5 without AlignedChunk) carries no chunk-info array.
  // RAFS v5 (FsVersion "5"): no `--features blob-toc` (builder.go:104-110),
  // so no TOC and no blob.meta entries; the bootstrap follows image.blob.
  const bool v6 = fs_version == 6;
  bool aligned = true;
  for (const RafsV6ChunkInfo &c : b.chunks)
    if (c.blob_index == st.own_blob_index && (c.uncompressed_offset & 4095)) aligned = false;
  uint64_t meta_entries = 0;
  if (k && aligned && v6) {
    std::vector<uint64_t> ci(3 * k, 0);
    std::vector<uint8_t> dig(32 * k);
    for (const RafsV6ChunkInfo &c : b.chunks) {
      if (c.blob_index != st.own_blob_index) continue;
      const uint64_t x = c.index;
      if ((c.uncompressed_offset >> 12) > 0xFFFFFFFFull || c.compressed_offset >= (1ull << 40) ||
          c.compressed_size == 0 || c.compressed_size > (1u << 24))
        return host_fail(NGPU_EFORMAT, "pack: chunk %llu does not fit a blob.meta chunk entry",
                         (unsigned long long)x);
      ci[3 * x] = ((c.uncompressed_offset >> 12) & 0xFFFFFFFFull) |
                  (((uint64_t)(c.uncompressed_size - 1) & 0xFFFFFF) << 32) |
                  ((uint64_t)(c.flags & 1) << 56);  // CHUNK_V2_FLAG_COMPRESSED
      ci[3 * x + 1] = (c.compressed_offset & 0xFFFFFFFFFFull) |
                      ((uint64_t)(c.compressed_size - 1) << 40);
      if (zr) {  // CHUNK_V2_FLAG_ZRAN; data = checkpoint index << 32 | offset in its output (VERIFY)
        ci[3 * x] |= 0x2ull << 56;
        ci[3 * x + 2] = (uint64_t)zr->ctx[x] << 32 | zr->ctx_off[x];
      }
      memcpy(&dig[32 * x], c.block_id, 32);
    }
    // targz-ref: the checkpoint table and dictionaries follow the chunk-info
    // array inside blob.meta (ZranInflateContext records, VERIFY)
    const uint64_t ci_entries_len = ci.size() * 8;
    std::vector<uint8_t> ci_all;
    if (zr) {
      ci_all.assign((const uint8_t *)ci.data(), (const uint8_t *)ci.data() + ci_entries_len);
      ci_all.insert(ci_all.end(), zr->table.begin(), zr->table.end());
      ci_all.insert(ci_all.end(), zr->dicts.begin(), zr->dicts.end());
    }
    const uint8_t *ci_raw = zr ? ci_all.data() : (const uint8_t *)ci.data();
    const uint64_t ci_len = zr ? ci_all.size() : ci_entries_len;
    uint8_t ci_dig[32];
    sha256(ci_raw, ci_len, ci_dig);
    std::vector<uint8_t> z;
    // The array is compressed with the blob's own compressor when that shrinks
    // it, as the reference v6 fixture's lz4_block blob has its array
    // lz4_block-compressed (ci_compressor 1: 40,240 -> 35,949 B); the TOC
    // entry carries the same compressor (the Go reader opens zstd / none only,
    // convert_unix.go:219-276: an lz4_block blob's blob.meta is for nydusd).
    uint32_t ci_algo = 0, ci_flag = NGPU_COMPRESSOR_NONE;  // compress::Algorithm None = 0
    if (!zr && (kind == NGPU_COMPRESSOR_ZSTD || kind == NGPU_COMPRESSOR_LZ4_BLOCK)) {
      z.resize(compress_bound(kind, (uint32_t)ci_len));
      const uint64_t zl = compress_one(kind, 0, ci_raw, (uint32_t)ci_len, z.data(), z.size());
      if (zl) {
        z.resize(zl);
        ci_algo = kind == NGPU_COMPRESSOR_ZSTD ? 3 : 1;  // compress::Algorithm Zstd / Lz4Block
        ci_flag = kind;
      }
    }
    const uint8_t *ci_data = ci_flag == NGPU_COMPRESSOR_NONE ? ci_raw : z.data();
    const uint64_t ci_size = ci_flag == NGPU_COMPRESSOR_NONE ? ci_len : z.size();
    const uint64_t ci_off = blob_bytes + tail.size();
    uint8_t h[4096];
    memset(h, 0, sizeof h);
    const uint32_t magic = 0xB10BB10Bu;  // BLOB_CCT_MAGIC
    // BlobFeatures: ALIGNED | INLINED_FS_META | CHUNK_INFO_V2 | INLINED_CHUNK_DIGEST |
    // HAS_TAR_HEADER | HAS_TOC | CAP_TAR_TOC
    // (+ ZRAN 0x8 for targz-ref, VERIFY)
    const uint32_t feat = 0x1 | 0x2 | 0x4 | 0x20 | 0x10000000u | 0x20000000u | 0x40000000u |
                          (zr ? 0x8u : 0u);
    const uint32_t nent = (uint32_t)k;
    memcpy(h + 0, &magic, 4);
    memcpy(h + 4, &feat, 4);
    memcpy(h + 8, &ci_algo, 4);
    memcpy(h + 12, &nent, 4);
    memcpy(h + 16, &ci_off, 8);
    memcpy(h + 24, &ci_size, 8);
    memcpy(h + 32, &ci_len, 8);
    if (zr) {  // where the checkpoint table and dictionaries sit (offsets in the uncompressed blob.meta)
      const uint64_t zt_off = ci_entries_len, zt_size = zr->table.size(), zt_cnt = zr->n_points;
      const uint64_t zd_off = zt_off + zt_size, zd_size = zr->dicts.size();
      memcpy(h + 40, &zt_off, 8);
      memcpy(h + 48, &zt_size, 8);
      memcpy(h + 56, &zt_cnt, 8);
      memcpy(h + 64, &zd_off, 8);
      memcpy(h + 72, &zd_size, 8);
    }
    memcpy(h + 4088, &magic, 4);  // s_magic2
    uint8_t h_dig[32], d_dig[32];
    sha256(h, sizeof h, h_dig);
    sha256(dig.data(), dig.size(), d_dig);
    put(ci_data, ci_size);
    put(h, sizeof h);
    hdr("blob.meta", ci_size + sizeof h);
    toc_add("blob.meta", ci_flag, ci_dig, ci_off, ci_size, ci_len);
    toc_add("blob.meta.header", NGPU_COMPRESSOR_NONE, h_dig, ci_off + ci_size, sizeof h, sizeof h);
    const uint64_t d_off = blob_bytes + tail.size();
    put(dig.data(), dig.size());
    hdr("blob.digest", dig.size());
    toc_add("blob.digest", NGPU_COMPRESSOR_NONE, d_dig, d_off, dig.size(), dig.size());
    meta_entries = k;
    // the own blob's record points at its chunk-info array.  RafsV6Blob after
    // uncompressed_size ([nydus v2.3.0] rafs/src/metadata/layout/v6.rs,
    // VERIFY; its offsets pinned by the reference v6 fixture's record, whose
    // values are ci_compressor 1 (lz4_block), ci_offset = the blob's compressed
    // size, 35,949 / 40,240 compressed / uncompressed bytes = 2,515 x 16-B v1
    // entries): blob_toc_size u32 (0 with inlined meta), ci_compressor u32,
    // ci_offset, ci_compressed_size, ci_uncompressed_size u64, then the ToC /
    // meta digests and size (zero with inlined meta).  Its features are the
    // blob's, as in the chunk-info header.
    RafsV6BlobInfo &ob = b.blobs[st.own_blob_index];
    uint8_t *bm = ob.meta;
    const uint32_t toc_size = 0;
    memcpy(bm + offsetof(RafsV6BlobMeta, blob_toc_size), &toc_size, 4);
    memcpy(bm + offsetof(RafsV6BlobMeta, ci_compressor), &ci_algo, 4);
    memcpy(bm + offsetof(RafsV6BlobMeta, ci_offset), &ci_off, 8);
    memcpy(bm + offsetof(RafsV6BlobMeta, ci_compressed_size), &ci_size, 8);
    memcpy(bm + offsetof(RafsV6BlobMeta, ci_uncompressed_size), &ci_len, 8);
    ob.features = feat;
  }
  // image.boot: the inode tree of the layer (rafs.cpp), RAFS v5 or v6
  li.blobs = b.blobs;
  li.table = b.chunks;
  std::vector<uint8_t> boot;
  if (int rc = write_rafs(entries, li, &boot)) return m.rc = rc;
  sha256(boot.data(), boot.size(), boot_dig);
  const uint64_t boot_off = blob_bytes + tail.size();
  put(boot.data(), boot.size());
  hdr("image.boot", boot.size());
  toc_add("image.boot", NGPU_COMPRESSOR_NONE, boot_dig, boot_off, boot.size(), boot.size());
  const uint64_t toc_bytes = toc.size() * sizeof(TocEntry);
  memset(toc_dig, 0, sizeof toc_dig);
  if (v6) {
    sha256(toc.data(), toc_bytes, toc_dig);
    put(toc.data(), toc_bytes);
    hdr("rafs.blob.toc", toc_bytes);
  }
  m.stream_sha.update(tail.data(), tail.size());
  m.stream_sha.final(stream_dig);
  if ((m.rc = m.emit(tail.data(), tail.size()))) return m.rc;
  if (info) {
    memset(info, 0, sizeof *info);
    info->stream_bytes = m.written;
    info->blob_bytes = blob_bytes;
    info->bootstrap_bytes = boot.size();
    info->blob_chunks = k;
    info->compressed_chunks = m.compressed_chunks;
    info->dict_records = ndict;
    info->meta_entries = meta_entries;
    memcpy(info->stream_digest, stream_dig, 32);
    memcpy(info->blob_digest, zr ? zr->digest : blob_dig, 32);  // targz-ref: the gzip blob
    memcpy(info->toc_digest, toc_dig, 32);
  }
  return 0;
}

namespace {

// ---- UnpackEntry (convert_unix.go:162-320) ---------------------------------
struct Reader {
  ngpu_read_at_fn ra;
  void *ctx;
  uint64_t size;
  int read(void *buf, uint64_t n, uint64_t off) const {
    if (off > size || n > size - off) return host_fail(NGPU_EFORMAT, "read beyond end");
    uint8_t *p = (uint8_t *)buf;
    while (n) {
      const int64_t r = ra(ctx, p, n, off);
      if (r <= 0) return host_fail(NGPU_EIO, "read_at failed at %llu", (unsigned long long)off);
      p += r;
      off += (uint64_t)r;
      n -= (uint64_t)r;
    }
    return 0;
  }
};

// seekFileByTarHeader (convert_unix.go:162-213): walk headers from the tail.
int seek_by_tar_header(const Reader &r, const std::string &target, int64_t max_size,
                       uint64_t *off, uint64_t *len) {
  if (r.size < 512) return host_fail(NGPU_EFORMAT, "invalid nydus tar size %llu",
                                     (unsigned long long)r.size);
  int64_t cur = (int64_t)r.size - 512;
  for (;;) {
    uint8_t h[512];
    int rc = r.read(h, 512, (uint64_t)cur);
    if (rc) return rc;
    std::string name;
    int64_t sz;
    if (!read_header(h, &name, &sz)) return host_fail(NGPU_EFORMAT, "parse nydus tar header");
    if (cur < sz) return host_fail(NGPU_EFORMAT, "invalid nydus tar data, name %s, size %lld",
                                   name.c_str(), (long long)sz);
    if (name == target) {
      if (max_size >= 0 && sz > max_size)
        return host_fail(NGPU_EFORMAT, "invalid nydus tar size %llu", (unsigned long long)r.size);
      *off = (uint64_t)(cur - sz);
      *len = (uint64_t)sz;
      return 0;
    }
    cur = cur - sz - 512;
    if (cur < 0) break;
  }
  return host_fail(NGPU_ENOTFOUND, "can't find target %s by seeking tar", target.c_str());
}

int copy_range(const Reader &r, uint64_t off, uint64_t len, ngpu_write_fn w, void *wctx) {
  std::vector<uint8_t> buf(std::min<uint64_t>(len, 8ull << 20) + 1);
  while (len) {
    const uint64_t k = std::min<uint64_t>(len, buf.size());
    int rc = r.read(buf.data(), k, off);
    if (rc) return rc;
    if (w && w(wctx, buf.data(), k) != 0) return host_fail(NGPU_EIO, "copy target data to writer");
    off += k;
    len -= k;
  }
  return 0;
}

// The zstd-compressed TOC entry at [off, off+len): decompressed as a stream
// (the reference reads it through zstd.NewReader over a SectionReader,
// convert_unix.go:255-270), so neither size field of an untrusted TOC sizes
// an allocation.
int copy_zstd(const Reader &r, uint64_t off, uint64_t len, const char *name, ngpu_write_fn w,
              void *wctx) {
  const Codecs &c = codecs();
  if (!c.zstd_create_dstream || !c.zstd_decompress_stream || !c.zstd_free_dstream)
    return host_fail(NGPU_EUNSUPP, "zstd unavailable");
  if (off > r.size || len > r.size - off)
    return host_fail(NGPU_EFORMAT, "entry %s runs past the end of the blob", name);
  void *ds = c.zstd_create_dstream();
  if (!ds) return host_fail(NGPU_ENOMEM, "zstd: no stream");
  std::vector<uint8_t> in(std::min<uint64_t>(len, 1u << 20) + 1), out(1u << 20);
  int rc = 0;
  // 0 between frames: an empty section is a clean EOF, as for the Go decoder
  size_t last = 0;
  while (len && !rc) {
    const uint64_t k = std::min<uint64_t>(len, in.size());
    if ((rc = r.read(in.data(), k, off))) break;
    off += k;
    len -= k;
    ZInBuf ib{in.data(), (size_t)k, 0};
    while (ib.pos < ib.size && !rc) {
      ZOutBuf ob{out.data(), out.size(), 0};
      last = c.zstd_decompress_stream(ds, &ob, &ib);
      if (c.zstd_is_error(last)) rc = host_fail(NGPU_EFORMAT, "zstd: bad entry %s", name);
      else if (w && ob.pos && w(wctx, out.data(), ob.pos) != 0) rc = host_fail(NGPU_EIO, "write failed");
    }
  }
  while (!rc && last != 0) {  // flush what the decoder still holds
    ZInBuf ib{in.data(), 0, 0};
    ZOutBuf ob{out.data(), out.size(), 0};
    last = c.zstd_decompress_stream(ds, &ob, &ib);
    if (c.zstd_is_error(last)) rc = host_fail(NGPU_EFORMAT, "zstd: bad entry %s", name);
    else if (ob.pos == 0 && last != 0) rc = host_fail(NGPU_EFORMAT, "zstd: truncated entry %s", name);
    else if (w && ob.pos && w(wctx, out.data(), ob.pos) != 0) rc = host_fail(NGPU_EIO, "write failed");
  }
  c.zstd_free_dstream(ds);
  return rc;
}

}  // namespace
}  // namespace ngpu

using namespace ngpu;

extern "C" {

const char *ngpu_host_error(void) { return host_error(); }

// A reader that went away (the Go side's pipe goroutine ending early, e.g.
// its dest failed) must fail the write with EPIPE, not raise SIGPIPE in a
// library thread: SIGPIPE is blocked in this thread around the write, and one
// it raised is taken back before the mask is restored.
int ngpu_write_fd(void *ctx, const void *buf, uint64_t len) {
  const int fd = (int)(intptr_t)ctx;
  const uint8_t *p = (const uint8_t *)buf;
  sigset_t pipe_set, old;
  sigemptyset(&pipe_set);
  sigaddset(&pipe_set, SIGPIPE);
  sigset_t pending;
  sigemptyset(&pending);
  sigpending(&pending);
  const bool was_pending = sigismember(&pending, SIGPIPE) == 1;
  pthread_sigmask(SIG_BLOCK, &pipe_set, &old);
  int rc = 0;
  while (len) {
    const ssize_t r = write(fd, p, len > (1ull << 30) ? (1ull << 30) : len);
    if (r < 0) {
      if (errno == EINTR) continue;
      const int en = errno;
      if (en == EPIPE && !was_pending) {
        const struct timespec zero = {0, 0};
        (void)sigtimedwait(&pipe_set, nullptr, &zero);  // ours: take it back
      }
      rc = host_fail(NGPU_EIO, "write(fd %d): %s", fd, strerror(en));
      break;
    }
    p += r;
    len -= (uint64_t)r;
  }
  pthread_sigmask(SIG_SETMASK, &old, nullptr);
  return rc;
}

int ngpu_blob_write(const void *data, uint64_t len, const ngpu_chunk *chunks,
                    const ngpu_result *results, uint64_t n, const ngpu_layer_stats *stats,
                    const ngpu_blob_options *opt, ngpu_write_fn w, void *ctx,
                    ngpu_blob_info *info) {
  const int rc = guarded([&]() -> int {
    if ((n && (!data || !chunks || !results)) || !stats || !opt || !w)
      return host_fail(NGPU_EINVAL, "ngpu_blob_write: bad argument");
    // 0 = the default 1 MiB (what the tar re-scan below uses); anything else
    // must be a power of two in [0x1000, 0x1000000] (types.go:76), as the
    // bootstrap writer divides by it
    ngpu_blob_options o = *opt;
    if (!o.chunk_size) o.chunk_size = 0x100000;
    if (o.chunk_size < 0x1000 || o.chunk_size > 0x1000000 || (o.chunk_size & (o.chunk_size - 1)))
      return host_fail(NGPU_EINVAL, "ngpu_blob_write: invalid chunk size 0x%x", o.chunk_size);
    opt = &o;
    std::vector<RafsV6BlobInfo> dict(opt->n_dict_blobs);
    if (opt->n_dict_blobs) {
      if (!opt->dict_blobs) return host_fail(NGPU_EINVAL, "ngpu_blob_write: dict_blobs is NULL");
      memcpy(dict.data(), opt->dict_blobs, dict.size() * sizeof(RafsV6BlobInfo));
    }
    if (opt->n_dict_chunks && !opt->dict_chunks)
      return host_fail(NGPU_EINVAL, "ngpu_blob_write: dict_chunks is NULL");
    std::vector<DictPlace> place(opt->n_dict_chunks);
    for (uint64_t i = 0; i < opt->n_dict_chunks; ++i) {
      RafsV6ChunkInfo r;
      memcpy(&r, (const uint8_t *)opt->dict_chunks + 80 * i, 80);
      place[i] = DictPlace{r.compressed_offset, r.compressed_size, r.flags};
    }
    // the layer tar's entries: the bootstrap's inode tree.  Walking the tar
    // must give back the caller's chunk list, or the tree would not match it.
    std::vector<TarEntry> entries;
    {
      struct Cmp : TarSink {
        const ngpu_chunk *ch;
        uint64_t n, k = 0;
        bool same = true;
        int chunk(uint64_t off, uint32_t l, uint32_t fi, uint64_t fo) override {
          if (k >= n || ch[k].offset != off || ch[k].length != l || ch[k].file_index != fi ||
              ch[k].file_offset != fo)
            same = false;
          ++k;
          return 0;
        }
        int data(const uint8_t *, uint64_t) override { return 0; }
      } cmp;
      cmp.ch = chunks;
      cmp.n = n;
      TarScanner sc(opt->chunk_size);
      sc.record(&entries);
      int rc = sc.feed((const uint8_t *)data, len, cmp);
      if (!rc) rc = sc.finish();
      if (rc || !cmp.same || cmp.k != n)
        return host_fail(NGPU_EINVAL,
                         "ngpu_blob_write: data is not the layer tar the %llu chunks were cut from "
                         "(chunk_size 0x%x)", (unsigned long long)n, opt->chunk_size);
    }
    BlobWriter bw(*opt, w, ctx, std::move(dict), place.data(), place.size());
    int rc = bw.init();
    if (rc) return rc;
    std::vector<const uint8_t *> src;
    std::vector<uint32_t> lens;
    const uint8_t *base = (const uint8_t *)data;
    for (uint64_t i = 0; i < n; ++i) {
      if (results[i].kind != NGPU_NEW) continue;
      if (chunks[i].offset > len || chunks[i].length > len - chunks[i].offset)
        return host_fail(NGPU_EINVAL, "ngpu_blob_write: chunk %llu out of bounds",
                         (unsigned long long)i);
      src.push_back(base + chunks[i].offset);
      lens.push_back(chunks[i].length);
    }
    // (the caller's data outlives bw: raw chunks are written from it in place)
    rc = bw.add(src.data(), lens.data(), src.size(), true);
    if (!rc) rc = bw.finish(chunks, results, n, *stats, entries, info);
    return rc;
  });
  if (rc == NGPU_ENOMEM) host_fail(rc, "ngpu_blob_write: out of memory");
  return rc;
}

int ngpu_unpack_entry(ngpu_read_at_fn ra, void *ctx, uint64_t size, const char *name,
                      ngpu_write_fn w, void *wctx, uint8_t *toc_entry_out) {
  const int rc = guarded([&]() -> int {
    if (!ra || !name) return host_fail(NGPU_EINVAL, "ngpu_unpack_entry: bad argument");
    Reader r{ra, ctx, size};
    if (toc_entry_out) memset(toc_entry_out, 0, sizeof(TocEntry));
    // seekFileByTOC (convert_unix.go:219-276)
    uint64_t toff = 0, tlen = 0;
    int rc = seek_by_tar_header(r, "rafs.blob.toc", 1 << 20, &toff, &tlen);
    if (rc == 0) {
      if (tlen % sizeof(TocEntry)) return host_fail(NGPU_EFORMAT, "invalid entries length %llu",
                                                    (unsigned long long)tlen);
      std::vector<TocEntry> toc(tlen / sizeof(TocEntry));
      if ((rc = r.read(toc.data(), tlen, toff))) return rc;
      for (const TocEntry &e : toc) {
        if (std::string(e.name, strnlen(e.name, sizeof e.name)) != name) continue;
        const uint32_t comp = e.flags & 0xf;
        if (comp == NGPU_COMPRESSOR_NONE) {
          rc = copy_range(r, e.compressed_offset, e.compressed_size, w, wctx);
        } else if (comp == NGPU_COMPRESSOR_ZSTD) {
          rc = copy_zstd(r, e.compressed_offset, e.compressed_size, name, w, wctx);
        } else {
          return host_fail(NGPU_EUNSUPP, "unsupported compressor %x", comp);
        }
        if (rc) return rc;
        if (toc_entry_out) memcpy(toc_entry_out, &e, sizeof e);
        return 0;
      }
    } else if (rc != NGPU_ENOTFOUND) {
      return rc;
    }
    // seekFile fallback: old rafs blob format, by tar header (convert_unix.go:302-320)
    uint64_t off = 0, len = 0;
    if ((rc = seek_by_tar_header(r, name, -1, &off, &len))) return rc;
    return copy_range(r, off, len, w, wctx);
  });
  if (rc == NGPU_ENOMEM) host_fail(rc, "ngpu_unpack_entry: out of memory");
  return rc;
}

namespace {
// Where an entry of the nydus stream lies: by the TOC (uncompressed entries)
// or by tar header.  *digest: the TOC's uncompressed sha256, or null.
int locate(const Reader &r, const char *name, uint64_t *off, uint64_t *len, bool *have_dig,
           uint8_t dig[32]) {
  *have_dig = false;
  uint64_t toff = 0, tlen = 0;
  int rc = seek_by_tar_header(r, "rafs.blob.toc", 1 << 20, &toff, &tlen);
  if (rc == 0 && tlen % sizeof(TocEntry) == 0) {
    std::vector<TocEntry> toc(tlen / sizeof(TocEntry));
    if ((rc = r.read(toc.data(), tlen, toff))) return rc;
    for (const TocEntry &e : toc) {
      if (std::string(e.name, strnlen(e.name, sizeof e.name)) != name) continue;
      if ((e.flags & 0xf) != NGPU_COMPRESSOR_NONE) break;  // by tar header below
      *off = e.compressed_offset;
      *len = e.compressed_size;
      memcpy(dig, e.uncompressed_digest, 32);
      *have_dig = true;
      if (*off > r.size || *len > r.size - *off) return host_fail(NGPU_EFORMAT, "bad TOC entry %s", name);
      return 0;
    }
  } else if (rc && rc != NGPU_ENOTFOUND) {
    return rc;
  }
  return seek_by_tar_header(r, name, -1, off, len);
}
}  // namespace

extern "C++" {
namespace ngpu {
int locate_layer(ngpu_read_at_fn ra, void *ctx, uint64_t size, LayerParts *out) {
  Reader r{ra, ctx, size};
  uint64_t boff, blen;
  bool bdig;
  uint8_t bd[32];
  int rc = locate(r, "image.boot", &boff, &blen, &bdig, bd);
  if (rc) return rc;
  if (blen > (8ull << 30)) return host_fail(NGPU_EFORMAT, "bootstrap of %llu bytes", (unsigned long long)blen);
  out->boot.resize(blen);
  if ((rc = r.read(out->boot.data(), blen, boff))) return rc;
  rc = locate(r, "image.blob", &out->data_off, &out->data_len, &out->have_digest, out->data_digest);
  out->has_data = rc == 0;
  if (rc == NGPU_ENOTFOUND) rc = 0;  // a layer with no chunk of its own
  return rc;
}

int own_blob_of(const std::vector<RafsV6BlobInfo> &blobs, const LayerParts &lp) {
  if (!lp.has_data) return -1;
  const std::string want = lp.have_digest ? hex(lp.data_digest, 32) : std::string();
  for (size_t i = 0; i < blobs.size(); ++i)
    if (!want.empty() && blob_id_of(blobs[i]) == want) return (int)i;
  for (size_t i = 0; i < blobs.size() && lp.data_len && want.empty(); ++i)
    if (blobs[i].compressed_size == lp.data_len) return (int)i;
  return -1;
}
}  // namespace ngpu
}  // extern "C++"

int ngpu_unpack(ngpu_read_at_fn ra, void *ctx, uint64_t size, ngpu_write_fn w, void *wctx) {
  const int rc = guarded([&]() -> int {
    if (!ra || !w) return host_fail(NGPU_EINVAL, "ngpu_unpack: bad argument");
    Reader r{ra, ctx, size};
    uint64_t boff, blen, doff, dlen;
    bool bdig, ddig;
    uint8_t bd[32], dd[32];
    int rc = locate(r, "image.boot", &boff, &blen, &bdig, bd);
    if (rc) return rc;
    if (blen > (8ull << 30)) return host_fail(NGPU_EFORMAT, "bootstrap of %llu bytes", (unsigned long long)blen);
    std::vector<uint8_t> boot(blen);
    if ((rc = r.read(boot.data(), blen, boff))) return rc;
    if ((rc = locate(r, "image.blob", &doff, &dlen, &ddig, dd))) return rc;
    std::vector<RafsNode> nodes;
    std::vector<RafsV6BlobInfo> blobs;
    uint32_t fsv = 0;
    if ((rc = read_rafs(boot.data(), boot.size(), &nodes, &blobs, &fsv))) return rc;
    // the layer's own blob: the one named by image.blob's digest (TOC), else
    // the one whose compressed size is image.blob's size
    int64_t own = -1;
    const std::string want = ddig ? hex(dd, 32) : std::string();
    for (size_t i = 0; i < blobs.size() && own < 0; ++i)
      if (!want.empty() && blob_id_of(blobs[i]) == want) own = (int64_t)i;
    for (size_t i = 0; i < blobs.size() && own < 0 && dlen && want.empty(); ++i)
      if (blobs[i].compressed_size == dlen) own = (int64_t)i;
    std::vector<uint8_t> out, cbuf, ubuf;
    std::unordered_map<uint64_t, std::string> first_path;  // ino -> first path (hardlinks)
    uint64_t flushed = 0;  // bytes already handed to w (tar padding is relative to the stream)
    auto flush = [&]() -> int {
      if (!out.empty() && w(wctx, out.data(), out.size()) != 0) return host_fail(NGPU_EIO, "unpack: write failed");
      flushed += out.size();
      out.clear();
      return 0;
    };
    for (const RafsNode &nd : nodes) {
      const uint32_t type = nd.mode & S_IFMT;
      char tf = '0';
      std::string link;
      uint64_t body = 0;
      if (type == S_IFDIR) tf = '5';
      else if (type == S_IFLNK) tf = '2', link = nd.link;
      else if (type == S_IFCHR) tf = '3';
      else if (type == S_IFBLK) tf = '4';
      else if (type == S_IFIFO) tf = '6';
      else if (type != S_IFREG) continue;  // sockets: not representable in a tar
      if (type != S_IFDIR && nd.nlink > 1) {
        auto it = first_path.find(nd.ino);
        if (it != first_path.end()) {
          tf = '1';
          link = it->second;
        } else {
          first_path.emplace(nd.ino, nd.path);
        }
      }
      if (tf == '0') body = nd.size;
      tar_entry_header(&out, nd, tf, link, body);
      if (tf == '0') {
        uint64_t done = 0;
        for (const RafsV6ChunkInfo &c : nd.chunks) {
          if ((int64_t)c.blob_index != own)
            return host_fail(NGPU_ENOTFOUND, "unpack: %s has a chunk in blob %u (%s), not in this layer",
                             nd.path.c_str(), c.blob_index,
                             c.blob_index < blobs.size() ? blob_id_of(blobs[c.blob_index]).c_str() : "?");
          if (c.compressed_offset > dlen || c.compressed_size > dlen - c.compressed_offset)
            return host_fail(NGPU_EFORMAT, "unpack: chunk of %s outside image.blob", nd.path.c_str());
          // sizes come from an untrusted bootstrap: a chunk never holds more
          // than the blob's chunk size or the file bytes still to emit, so
          // neither sizes the buffer past that
          const uint32_t bcs = blobs[own].chunk_size;
          if (c.uncompressed_size > nd.size - done || (bcs && c.uncompressed_size > bcs))
            return host_fail(NGPU_EFORMAT, "unpack: chunk of %s larger than its file or chunk size",
                             nd.path.c_str());
          cbuf.resize(c.compressed_size);
          if ((rc = r.read(cbuf.data(), c.compressed_size, doff + c.compressed_offset))) return rc;
          const uint8_t *data = cbuf.data();
          if (c.flags & 1) {  // compressed with the blob's algorithm
            ubuf.resize(c.uncompressed_size);
            if ((rc = decompress_chunk(blobs[own].compression_algo, cbuf.data(), c.compressed_size,
                                       ubuf.data(), c.uncompressed_size)))
              return rc;
            data = ubuf.data();
          } else if (c.compressed_size != c.uncompressed_size) {
            return host_fail(NGPU_EFORMAT, "unpack: raw chunk of %s with csize != usize", nd.path.c_str());
          }
          const uint64_t take = std::min<uint64_t>(c.uncompressed_size, nd.size - done);
          out.insert(out.end(), data, data + take);
          done += take;
          if (out.size() >= (8u << 20) && (rc = flush())) return rc;
        }
        if (done != nd.size) return host_fail(NGPU_EFORMAT, "unpack: %s: %llu of %llu bytes in its chunks",
                                              nd.path.c_str(), (unsigned long long)done,
                                              (unsigned long long)nd.size);
        out.resize(out.size() + (512 - (flushed + out.size()) % 512) % 512, 0);
      }
      if (out.size() >= (8u << 20) && (rc = flush())) return rc;
    }
    out.resize(out.size() + 1024, 0);  // end of archive: two zero blocks
    return flush();
  });
  if (rc == NGPU_ENOMEM) host_fail(rc, "ngpu_unpack: out of memory");
  return rc;
}

// 64 hex chars (an optional "sha256:" prefix) -> 32 bytes
static bool unhex32(const char *s, uint8_t out[32]) {
  if (!strncmp(s, "sha256:", 7)) s += 7;
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 32; ++i) {
    int v = 0;
    for (int k = 0; k < 2; ++k) {
      const char c = s[2 * i + k];
      const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10
                  : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
      if (d < 0) return false;
      v = v * 16 + d;
    }
    out[i] = (uint8_t)v;
  }
  return true;
}

int ngpu_merge_ex(const void *const *bootstraps, const uint64_t *sizes,
                  const char *const *layer_digests, uint64_t n, const void *dict_bootstrap,
                  uint64_t dict_size, const ngpu_merge_options *opt, ngpu_write_fn w, void *ctx,
                  char **blob_ids_out) {
  return ngpu_merge_ex2(bootstraps, sizes, layer_digests, n, dict_bootstrap, dict_size, opt,
                        nullptr, nullptr, nullptr, w, ctx, blob_ids_out);
}

int ngpu_merge_ex2(const void *const *bootstraps, const uint64_t *sizes,
                   const char *const *layer_digests, uint64_t n, const void *dict_bootstrap,
                   uint64_t dict_size, const ngpu_merge_options *opt,
                   const char *const *rafs_blob_digests, const uint64_t *rafs_blob_sizes,
                   const char *const *rafs_blob_toc_digests, ngpu_write_fn w, void *ctx,
                   char **blob_ids_out) {
  const int rc = guarded([&]() -> int {
    if ((n && (!bootstraps || !sizes)) || !blob_ids_out ||
        (opt && opt->parent_size && !opt->parent_bootstrap))
      return host_fail(NGPU_EINVAL, "ngpu_merge: bad argument");
    *blob_ids_out = nullptr;
    std::vector<std::string> dict_ids;
    if (dict_bootstrap) {  // --chunk-dict bootstrap=P: RAFS v6 or v5
      const uint8_t *dp = (const uint8_t *)dict_bootstrap;
      uint32_t m5 = 0;
      if (dict_size >= 4) memcpy(&m5, dp, 4);
      if (m5 == kRafsV5Magic) {
        uint32_t dg, cs;
        std::vector<uint8_t> recs, blobs;
        if (int rc = parse_v5_bootstrap(dp, dict_size, &dg, &cs, &recs, &blobs)) return rc;
        for (size_t i = 0; i + sizeof(RafsV6BlobInfo) <= blobs.size(); i += sizeof(RafsV6BlobInfo)) {
          RafsV6BlobInfo b;
          memcpy(&b, blobs.data() + i, sizeof b);
          dict_ids.push_back(blob_id_of(b));
        }
      } else {
        Bootstrap d;
        if (int rc = parse_bootstrap(dp, dict_size, &d, false)) return rc;
        for (auto &b : d.blobs) dict_ids.push_back(blob_id_of(b));
      }
    }
    std::vector<MergeInput> in;
    if (opt && opt->parent_bootstrap) {
      MergeInput m;
      m.p = (const uint8_t *)opt->parent_bootstrap;
      m.n = opt->parent_size;
      m.parent = true;
      in.push_back(m);
    }
    for (uint64_t l = 0; l < n; ++l) {
      MergeInput m;
      m.p = (const uint8_t *)bootstraps[l];
      m.n = sizes[l];
      // A layer's own (non-dict) blob is named after the layer: the digest of
      // its whole nydus tar stream, which Merge receives as Layer.Digest and
      // uses as the bootstrap file name (convert_unix.go:567-573, 595-599).
      if (layer_digests && layer_digests[l]) m.own_name = layer_digests[l];
      if (rafs_blob_digests && rafs_blob_digests[l]) {  // targz-ref layer
        if (!rafs_blob_sizes || !rafs_blob_toc_digests || !rafs_blob_toc_digests[l] ||
            !unhex32(rafs_blob_digests[l], m.rafs_blob_digest) ||
            !unhex32(rafs_blob_toc_digests[l], m.toc_digest))
          return host_fail(NGPU_EINVAL, "ngpu_merge: layer %llu: bad RAFS blob / TOC digest",
                           (unsigned long long)l);
        m.rafs_blob_size = rafs_blob_sizes[l];
        m.ref = true;
      }
      in.push_back(m);
    }
    std::vector<uint8_t> boot;
    std::vector<std::string> ids;
    const std::string pf = opt && opt->prefetch_patterns ? opt->prefetch_patterns : "";
    if (int rc = merge_rafs(in, dict_ids, pf, &boot, &ids)) return rc;
    if (w && w(ctx, boot.data(), boot.size()) != 0) return host_fail(NGPU_EIO, "write failed");
    std::string s;
    for (size_t i = 0; i < ids.size(); ++i) s += (i ? "," : "") + ids[i];
    char *o = (char *)malloc(s.size() + 1);
    if (!o) return NGPU_ENOMEM;
    memcpy(o, s.c_str(), s.size() + 1);
    *blob_ids_out = o;
    return 0;
  });
  if (rc == NGPU_ENOMEM) host_fail(rc, "ngpu_merge: out of memory");
  return rc;
}

int ngpu_rafs_dump(const void *bootstrap, uint64_t size, ngpu_write_fn w, void *ctx) {
  const int rc = guarded([&]() -> int {
    if (!bootstrap || !w) return host_fail(NGPU_EINVAL, "ngpu_rafs_dump: bad argument");
    std::string js;
    if (int rc = rafs_dump_json((const uint8_t *)bootstrap, size, &js)) return rc;
    if (w(ctx, js.data(), js.size()) != 0) return host_fail(NGPU_EIO, "ngpu_rafs_dump: write failed");
    return 0;
  });
  if (rc == NGPU_ENOMEM) host_fail(rc, "ngpu_rafs_dump: out of memory");
  return rc;
}

int ngpu_merge(const void *const *bootstraps, const uint64_t *sizes,
               const char *const *layer_digests, uint64_t n, const void *dict_bootstrap,
               uint64_t dict_size, ngpu_write_fn w, void *ctx, char **blob_ids_out) {
  return ngpu_merge_ex(bootstraps, sizes, layer_digests, n, dict_bootstrap, dict_size, nullptr, w,
                       ctx, blob_ids_out);
}

}  // extern "C"
