// node.hip — one process driving the GPUs of a node, and
// node chunk dicts: partitioned by digest prefix, or replicated.
//
// The reference converts layers concurrently in one process (goroutines,
// pkg/converter/convert_unix.go:467-538) and hands each to its own
// nydus-image; the chunk dict is loaded by every one of them.  Here a node
// keeps one engine per GPU and one dict for all of them.  A partitioned dict
// keeps the entries whose digest prefix maps to device o on device o
// (owner = ((d[0] << 8 | d[1]) * n) >> 16, nydus_gpu/dist.py's rule), in
// global table order, with their global entry ids, so "first entry wins" and
// the DICT results are the same as with the whole dict on one GPU.
//
// The exchange (the north star's digest-prefix all-to-all, in-process): the
// requester packs its chunk digests (n x 32 B), every owner receives them over
// xGMI with hipMemcpyPeerAsync, probes the rows it owns, and its hit array
// (n x 24 B) goes back the same way; the requester merges the W arrays by
// owner.  Every (owner, requester) pair has its own channel -- probe stream,
// buffers and cached done event on the owner -- so W requesters exchange at
// once with no shared lock, buffer or queue between them; an owner's W
// probes run concurrently on its CUs.  Copies, not peer loads/stores from kernels:
// the DMA engines keep coarse-grained HBM coherent across the GPUs, and the
// payload is tiny (16K chunks of a 16 GiB layer = 512 KiB out, 384 KiB back
// per owner), so the exchange is latency-bound, not link-bound.
//
// The node step (ngpu_node_process_step) is the bulk form: every part at
// once, one all-to-all-v of digests and one of hits, over RCCL or peer
// copies.  It routes into padded per-owner segments (a2a_plan.hpp) so that
// no transfer size depends on a device-side count: the counts cross in band
// and the whole step enqueues without a host wait.
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>

#include <rccl/rccl.h>

#include "a2a_plan.hpp"
#include "dict_retire_plan.hpp"
#include "engine_internal.hpp"
#include "node_distill_plan.hpp"
#include "node_fold_plan.hpp"
#include "node_remode_plan.hpp"
#include "node_retire_plan.hpp"

using namespace ngpu;

namespace {
// Buffers of one part of a node step (ngpu_node_process_step), on its device.
struct StepBuf {
  uint8_t *xq = nullptr;          // its digests bucketed by owner, padded: W x n rows of 32 B
  uint32_t *xrow = nullptr;       // their row ids (~0: padding)
  ngpu_dict_hit *sh = nullptr;    // hits returned, same (owner-bucketed, padded) order
  ngpu_dict_hit *hits = nullptr;  // hits by row
  uint64_t cap = 0;               // rows of xq / xrow / sh / hits
  uint8_t *rq = nullptr;          // digests it received as owner (R x 32)
  ngpu_dict_hit *rh = nullptr;    // its hits for them
  uint64_t rcap = 0;
  uint32_t *cnt = nullptr;        // 128 u32: per-owner counts (+ scatter cursors)
  uint32_t *rcnt = nullptr;       // 64 u32: as owner, each requester's count (in band)
  hipEvent_t counted = nullptr, sent = nullptr, returned = nullptr, done = nullptr;
};
}  // namespace

struct ngpu_node {
  std::vector<ngpu_engine *> eng;  // one per listed device (a reference each)
  std::vector<int> dev;
  std::atomic<uint64_t> rr{0};     // where a Pack's least-loaded search starts (ties)
  std::mutex place_mu;             // one placement at a time: concurrent opens spread evenly
  // node dicts opened by path (one reference each; ngpu_node_dict_open)
  std::vector<ngpu_dict *> dict_cache;
  std::mutex cache_mu;
  bool peer_ok = true;             // every pair of distinct devices has peer access
  // node steps (ngpu_node_process_step): one at a time, buffers per part,
  // the RCCL communicator of the node's devices once a step asked for it
  std::mutex step_mu;
  std::vector<StepBuf> sb;
  bool stepped = false;            // sb[*].done recorded by a previous step
  std::vector<ncclComm_t> comms;
};

namespace ngpu {

static void free_io(ngpu_dict::PartIO &io, int device) {
  DeviceGuard g(device);
  if (io.stream) (void)hipStreamSynchronize(io.stream);
  if (io.q) (void)hipFree(io.q);
  if (io.h) (void)hipFree(io.h);
  io.q = nullptr;
  io.h = nullptr;
  io.cap = 0;
}

// The requester's channel set: found (or added) under req_mu, which is held
// for the lookup only -- the enqueue itself runs under the requester's own mu.
static ngpu_dict::Requester *requester_of(ngpu_engine *e, ngpu_dict *d) {
  std::lock_guard<std::mutex> g(d->req_mu);
  for (auto &r : d->req)
    if (r->engine_uid == e->uid) return r.get();
  d->req.emplace_back(new ngpu_dict::Requester());
  ngpu_dict::Requester *r = d->req.back().get();
  r->engine_uid = e->uid;
  r->device = e->device;
  r->io.resize(d->parts.size());
  return r;
}

// One owner's channel for this requester: stream, buffers for n rows and the
// done event on the owner's device (created once, reused by every call).
static int channel_ready(ngpu_engine *e, ngpu_dict::PartIO &io, int device, uint64_t n,
                         uint64_t cap) {
  DeviceGuard dg(device);
  if (!io.stream && hipStreamCreateWithFlags(&io.stream, hipStreamNonBlocking) != hipSuccess)
    return fail(e, NGPU_EHIP, "node dict: probe stream on device %d", device);
  if (!io.done && hipEventCreateWithFlags(&io.done, hipEventDisableTiming) != hipSuccess)
    return fail(e, NGPU_EHIP, "node dict: exchange event on device %d", device);
  if (n > io.cap) {
    free_io(io, device);  // the stream's earlier exchanges finish first
    if (hipMalloc((void **)&io.q, cap * 32) != hipSuccess ||
        hipMalloc((void **)&io.h, cap * sizeof(ngpu_dict_hit)) != hipSuccess) {
      free_io(io, device);
      return fail(e, NGPU_ENOMEM, "node dict: exchange buffers on device %d", device);
    }
    io.cap = cap;
  }
  return 0;
}

// The routed exchange (ABI 4): the requester buckets its n digests by owner in
// its own HBM (ws.xq rows, ws.xrow row ids, ws.xcnt counts); owner o's probe
// kernel, launched on o's device after the requester's `ready` event, reads
// only its own segment (peer loads over xGMI) and stores each hit at its row
// in the requester's ws.xhits (peer stores).  The requester's stream waits for
// every owner's `done`.  Bytes over the links per call: n x 36 out and n x 24
// back in total, against W x n x 56 for the copy exchange below it.
// Reuse is stream-ordered: the next call's routing on s runs after this call's
// waits on every `done`, so no owner still reads ws.xq when it is rewritten.
static int routed_hits(ngpu_engine *e, ngpu_dict *d, const uint8_t *digests, uint64_t stride,
                       uint64_t n, hipStream_t s, const ngpu_dict_hit **hits) {
  const uint32_t W = (uint32_t)d->parts.size();
  Workspace &ws = e->cur->ws;
  const bool regrow = n > ws.cap_x || !ws.xq || !ws.xrow || !ws.xhits;
  if (regrow && (ws.xq || ws.xrow || ws.xhits))
    if (int rc = slot_quiesce(e)) return rc;  // no buffer freed under a running stage
  if (regrow) {
    if (ws.xq) (void)hipFree(ws.xq), ws.xq = nullptr;
    if (ws.xhits) (void)hipFree(ws.xhits), ws.xhits = nullptr;
    if (ws.xrow) (void)hipFree(ws.xrow), ws.xrow = nullptr;
    const uint64_t c = next_pow2(n < 1024 ? 1024 : n);
    HIP_TRY(e, hipMalloc((void **)&ws.xq, c * 32));
    HIP_TRY(e, hipMalloc((void **)&ws.xhits, c * sizeof(ngpu_dict_hit)));
    HIP_TRY(e, hipMalloc((void **)&ws.xrow, c * 4));
    ws.cap_x = c;
  }
  if (!ws.xcnt) HIP_TRY(e, hipMalloc((void **)&ws.xcnt, 128 * sizeof(uint32_t)));
  *hits = ws.xhits;
  if (n == 0) return 0;
  ngpu_dict::Requester *r = requester_of(e, d);
  std::lock_guard<std::mutex> g(r->mu);  // this requester's channels only
  if (!r->ready) HIP_TRY(e, hipEventCreateWithFlags(&r->ready, hipEventDisableTiming));
  launch_route(digests, stride, n, W, 0, ws.xcnt, ws.xq, ws.xrow, s);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipEventRecord(r->ready, s));
  int rc = 0;
  uint32_t sent = 0;
  for (uint32_t o = 0; o < W && !rc; ++o, ++sent) {
    ngpu_dict *p = d->parts[o];
    ngpu_dict::PartIO &io = r->io[o];
    if ((rc = channel_ready(e, io, p->device, 0, 0))) break;
    DeviceGuard dg(p->device);
    if (hipStreamWaitEvent(io.stream, r->ready, 0) != hipSuccess) {
      rc = fail(e, NGPU_EHIP, "node dict: wait on the requester failed (device %d)", p->device);
      break;
    }
    launch_dict_probe_routed(ws.xq, ws.xrow, ws.xcnt, n, o, p->dev, ws.xhits, io.stream);
    if (hipGetLastError() != hipSuccess || hipEventRecord(io.done, io.stream) != hipSuccess)
      rc = fail(e, NGPU_EHIP, "node dict: routed probe on device %d failed", p->device);
  }
  // the requester's stream waits for every owner it enqueued, even on failure,
  // so no later stage reuses ws.xq / ws.xhits under a probe still in flight
  for (uint32_t o = 0; o < sent && o < W; ++o)
    if (r->io[o].done && hipStreamWaitEvent(s, r->io[o].done, 0) != hipSuccess && !rc)
      rc = fail(e, NGPU_EHIP, "node dict: cross-device wait failed");
  return rc;
}

int node_dict_hits(ngpu_engine *e, ngpu_dict *d, const uint8_t *digests, uint64_t stride,
                   uint64_t n, hipStream_t s, const ngpu_dict_hit **hits, ngpu_dict **replica) {
  *hits = nullptr;
  *replica = nullptr;
  if (d->replicated) {  // no exchange: the copy on this engine's device
    for (ngpu_dict *p : d->parts)
      if (p->device == e->device) {
        *replica = p;
        return 0;
      }
    return fail(e, NGPU_EINVAL, "node chunk dict has no replica on device %d", e->device);
  }
  const uint32_t W = (uint32_t)d->parts.size();
  Workspace &ws = e->cur->ws;  // the dedup stage's slot (use_slot)
  if (d->routed) return routed_hits(e, d, digests, stride, n, s, hits);
  if (((n > ws.cap_x && ws.xq) || ((uint64_t)W * n > ws.cap_xparts && ws.xparts)))
    if (int rc = slot_quiesce(e)) return rc;  // no buffer freed under a running stage
  if (n > ws.cap_x || !ws.xq) {
    if (ws.xq) (void)hipFree(ws.xq), ws.xq = nullptr;
    if (ws.xhits) (void)hipFree(ws.xhits), ws.xhits = nullptr;
    // cap_x is the routed exchange's too: its row ids go with the old size, so
    // that it allocates all three again and never routes n <= cap_x rows into a
    // shorter xrow
    if (ws.xrow) (void)hipFree(ws.xrow), ws.xrow = nullptr;
    const uint64_t c = next_pow2(n < 1024 ? 1024 : n);
    HIP_TRY(e, hipMalloc((void **)&ws.xq, c * 32));
    HIP_TRY(e, hipMalloc((void **)&ws.xhits, c * sizeof(ngpu_dict_hit)));
    ws.cap_x = c;
  }
  if ((uint64_t)W * n > ws.cap_xparts || !ws.xparts) {
    if (ws.xparts) (void)hipFree(ws.xparts), ws.xparts = nullptr;
    const uint64_t c = (uint64_t)W * ws.cap_x;
    HIP_TRY(e, hipMalloc((void **)&ws.xparts, c * sizeof(ngpu_dict_hit)));
    ws.cap_xparts = c;
  }
  *hits = ws.xhits;
  if (n == 0) return 0;
  ngpu_dict::Requester *r = requester_of(e, d);
  std::lock_guard<std::mutex> g(r->mu);  // this requester's channels only
  if (!r->ready) HIP_TRY(e, hipEventCreateWithFlags(&r->ready, hipEventDisableTiming));
  launch_pack_digests(digests, stride, n, ws.xq, s);
  HIP_TRY(e, hipEventRecord(r->ready, s));
  int rc = 0;
  uint32_t sent = 0;
  for (uint32_t o = 0; o < W && !rc; ++o, ++sent) {
    ngpu_dict *p = d->parts[o];
    ngpu_dict::PartIO &io = r->io[o];
    if ((rc = channel_ready(e, io, p->device, n, ws.cap_x))) break;
    DeviceGuard dg(p->device);
    const bool ok =
        hipStreamWaitEvent(io.stream, r->ready, 0) == hipSuccess &&
        hipMemcpyPeerAsync(io.q, p->device, ws.xq, e->device, n * 32, io.stream) == hipSuccess;
    if (ok) launch_dict_probe_owned(io.q, n, o, W, p->dev, io.h, io.stream);
    if (!ok || hipGetLastError() != hipSuccess ||
        hipMemcpyPeerAsync(ws.xparts + (uint64_t)o * n, e->device, io.h, p->device,
                           n * sizeof(ngpu_dict_hit), io.stream) != hipSuccess ||
        hipEventRecord(io.done, io.stream) != hipSuccess)
      rc = fail(e, NGPU_EHIP, "node dict: exchange with device %d failed", p->device);
  }
  // the requester's stream waits for every owner it enqueued, even on failure,
  // so no later stage reuses ws.xq / ws.xparts under a copy still in flight
  for (uint32_t o = 0; o < sent && o < W; ++o)
    if (r->io[o].done && hipStreamWaitEvent(s, r->io[o].done, 0) != hipSuccess && !rc)
      rc = fail(e, NGPU_EHIP, "node dict: cross-device wait failed");
  if (rc) return rc;
  launch_hits_merge(ws.xq, n, W, ws.xparts, ws.xhits, s);
  HIP_TRY(e, hipGetLastError());
  return 0;
}

namespace {

// base is a dict of this node: one part per device, in the node's order, and
// usable by its engines.  what: "extend", "retire", "fold".
int node_dict_base_check(ngpu_node *node, const ngpu_dict *base, const char *what) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (base->parts.empty())
    return fail(e0, NGPU_EINVAL, "node dict %s: not a node dict (ngpu_dict_%s takes it)", what, what);
  bool ours = base->parts.size() == W;
  for (uint32_t o = 0; ours && o < W; ++o) ours = base->parts[o]->device == node->eng[o]->device;
  if (!ours) return fail(e0, NGPU_EINVAL, "node dict %s: dict of another node", what);
  return dict_check(e0, base);
}

// k host records by owner part, in table order, with their global ids gid0 + position
// (part_recs, gid: W empty vectors).
void node_partition_records(const uint8_t *recs, uint64_t k, uint32_t W, uint64_t gid0,
                            std::vector<std::vector<uint8_t>> *part_recs,
                            std::vector<std::vector<uint32_t>> *gid) {
  for (uint64_t i = 0; i < k; ++i) {
    const uint32_t o = owner_of(recs + 80 * i, W);
    (*part_recs)[o].insert((*part_recs)[o].end(), recs + 80 * i, recs + 80 * (i + 1));
    (*gid)[o].push_back((uint32_t)(gid0 + i));
  }
}

// The `mode` of ngpu_node_dict_create and ngpu_node_dict_remode: replicated or
// partitioned, and the exchange a partitioned dict runs.
int node_dict_mode(ngpu_node *node, uint32_t mode, bool *replicated, bool *routed) {
  ngpu_engine *e0 = node->eng[0];
  const bool want_routed = (mode & NGPU_NODE_EXCHANGE_ROUTED) != 0;
  if ((mode & NGPU_NODE_EXCHANGE_COPY) && want_routed)
    return fail(e0, NGPU_EINVAL, "node dict: copy and routed exchange both asked for");
  mode &= ~(NGPU_NODE_EXCHANGE_COPY | NGPU_NODE_EXCHANGE_ROUTED);
  if (mode != NGPU_NODE_DICT_PARTITION && mode != NGPU_NODE_DICT_REPLICATE)
    return fail(e0, NGPU_EINVAL, "bad node dict mode %u", mode);
  *replicated = mode == NGPU_NODE_DICT_REPLICATE;
  // the copy exchange (DMA peer copies) unless the routed one was asked for
  // and every pair of devices has peer access (its kernels reach the
  // requester's HBM): the routed exchange's peer stores have not met two
  // distinct GPUs yet
  *routed = !*replicated && want_routed && node->peer_ok;
  return 0;
}

// A node dict over records in host memory (each part built on its device's
// own build stream, no engine lock held).
int node_dict_build(ngpu_node *node, const uint8_t *recs, uint64_t m, const uint8_t *blobs,
                    uint32_t n_blobs, uint32_t mode, ngpu_dict **out) {
  ngpu_engine *e0 = node->eng[0];
  bool replicated = false, routed = false;
  if (int rc = node_dict_mode(node, mode, &replicated, &routed)) return rc;
  if (m >= 0xFFFFFFFFull) return fail(e0, NGPU_EINVAL, "chunk dict too large");
  uint32_t nb = 0;
  if (int rc = records_blob_count(e0, recs, m, n_blobs, &nb)) return rc;
  ngpu_dict *d = dict_new(e0);
  d->replicated = replicated;
  d->routed = routed;
  d->dev.m = m;
  d->dev.n_blobs = nb;
  // the global handle sits on a storage of placement rows only
  if (int rc = dict_place_extend(e0, nullptr, recs, m, d)) {
    dict_unref(d);
    return rc;
  }
  if (blobs && n_blobs) d->blob_table.assign(blobs, blobs + 256ull * n_blobs);
  const uint32_t W = (uint32_t)node->eng.size();
  // partition: rows per owner in global table order, with their global ids
  std::vector<std::vector<uint8_t>> part_recs(W);
  std::vector<std::vector<uint32_t>> gid(W);
  if (!d->replicated) node_partition_records(recs, m, W, 0, &part_recs, &gid);
  int rc = 0;
  for (uint32_t o = 0; o < W && !rc; ++o) {
    ngpu_engine *e = node->eng[o];
    DeviceGuard dg(e->device);
    ngpu_dict *p = nullptr;
    const uint8_t *pr = d->replicated ? recs : part_recs[o].data();
    const uint64_t pm = d->replicated ? m : gid[o].size();
    if ((rc = dict_from_records(e, pr, pm, blobs, nb, &p, d->replicated ? nullptr : gid[o].data())))
      break;
    p->dev.n_blobs = nb;
    // the global table (d's storage) answers the writer
    free(p->st->place);
    p->st->place = nullptr;
    p->has_place = false;
    d->parts.push_back(p);
  }
  if (rc) {
    dict_unref(d);
    return rc;
  }
  *out = d;
  return 0;
}

// base followed by k more records: every part extended in place or onto a new
// storage as its own plan says (a partitioned part gets the records it owns,
// with global ids m + position; a replica gets all of them), the global
// placement rows likewise.
int node_dict_extend(ngpu_node *node, ngpu_dict *base, const uint8_t *recs, uint64_t k,
                     const uint8_t *blobs, uint32_t n_blobs, ngpu_dict **out) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (int rc = node_dict_base_check(node, base, "extend")) return rc;
  uint32_t nb = 0;
  bool with_table = false;
  if (int rc = dict_extend_check(e0, base, recs, k, blobs, n_blobs, &nb, &with_table)) return rc;
  const uint64_t m = base->dev.m;
  ngpu_dict *d = dict_derive(base);
  d->dev.m = m + k;
  d->dev.n_blobs = nb;
  int rc = dict_place_extend(e0, base, recs, k, d);
  std::vector<std::vector<uint8_t>> part_recs(W);
  std::vector<std::vector<uint32_t>> gid(W);
  if (!rc && !d->replicated) node_partition_records(recs, k, W, m, &part_recs, &gid);
  for (uint32_t o = 0; o < W && !rc; ++o) {
    ngpu_dict *p = nullptr;
    const uint8_t *pr = d->replicated ? recs : part_recs[o].data();
    const uint64_t pk = d->replicated ? k : gid[o].size();
    if ((rc = dict_extend_records(node->eng[o], base->parts[o], pr, pk, base->dev.n_blobs, nb,
                                  d->replicated ? nullptr : gid[o].data(), false, &p)))
      break;
    d->parts.push_back(p);
  }
  if (rc) {
    dict_unref(d);
    return rc;
  }
  dict_merge_blob_table(d, base, with_table, blobs, n_blobs);
  *out = d;
  return 0;
}

// base without the records of the listed blobs (dict.hip "dict retire"): every
// replica retired alike, the global placement rows compacted by part 0's keep
// words.  Partitioned dicts are refused here (the answer ngpu_node_dict_retire
// has always given): node_dict_retire_parts below retires them.
int node_dict_retire(ngpu_node *node, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                     ngpu_dict **out) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (int rc = node_dict_base_check(node, base, "retire")) return rc;
  const DictRetirePlan plan = dict_retire_plan(base->dev.n_blobs, blobs, n);
  if (!plan.ok)
    return fail(e0, NGPU_EINVAL, "node dict retire: blob %u of a dict of %u blobs", plan.bad,
                base->dev.n_blobs);
  if (!base->replicated)
    return fail(e0, NGPU_EUNSUPP,
                "node dict retire: partitioned node dicts are not supported yet (replicated ones are)");
  ngpu_dict *d = dict_derive(base);
  DictKeep keep;
  int rc = 0;
  for (uint32_t o = 0; o < W && !rc; ++o) {
    ngpu_dict *p = nullptr;
    if ((rc = dict_retire_records(node->eng[o], base->parts[o], plan.bitmap, plan.remap, plan.n_kept,
                                  nullptr, o == 0 ? &keep : nullptr, &p)))
      break;
    if (o && p->dev.m != d->parts[0]->dev.m) {
      dict_unref(p);
      rc = fail(e0, NGPU_EINVAL, "node dict retire: the replicas differ");
      break;
    }
    d->parts.push_back(p);
  }
  if (!rc) {
    const uint64_t m = base->dev.m, s = d->parts[0]->dev.m;
    d->dev.m = s;
    d->dev.n_blobs = plan.n_kept;
    // the global handle: placement rows only (if base keeps any), with a fork's room
    const DictPlace *rows = base->place();
    const uint64_t cap = dict_retire_rec_cap(s);
    if (!(rc = storage_alloc_place_only(e0, rows && s ? cap : 0, &d->st))) {
      d->st->rec_cap = cap;
      d->st->used = s;
      if (rows && s) {
        dict_retire_place(keep, m, rows, d->st->place, s);
        d->has_place = true;
      }
    }
  }
  if (rc) {
    dict_unref(d);
    return rc;
  }
  d->blob_table = dict_retire_blob_table(base->blob_table, plan.remap);
  *out = d;
  return 0;
}

// base with one row per digest (dict.hip "dict distill"): every replica distilled
// alike, the global placement rows compacted by part 0's keep words, as
// node_dict_retire does.  want_out false: the counts of part 0 alone.
int node_dict_distill(ngpu_node *node, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                      ngpu_dict **out, ngpu_dict_distill_info *info) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (int rc = node_dict_base_check(node, base, "distill")) return rc;
  if ((flags & NGPU_DICT_DISTILL_MERGE_BLOB_IDS) && base->dev.m && base->blob_table.empty())
    return fail(e0, NGPU_EINVAL,
                "node dict distill: blob ids are merged by the blob table, the dict has none");
  if (!base->replicated)
    return fail(e0, NGPU_EUNSUPP,
                "node dict distill: partitioned node dicts are not supported yet (replicated ones are)");
  DictDistilled res;
  if (!out) {
    if (int rc = dict_distill_records(e0, base->parts[0], base->blob_table, min_refs, flags, nullptr,
                                      nullptr, false, &res, nullptr))
      return rc;
    if (info) *info = res.info;
    return 0;
  }
  ngpu_dict *d = dict_derive(base);
  DictKeep keep;
  int rc = 0;
  for (uint32_t o = 0; o < W && !rc; ++o) {
    ngpu_dict *p = nullptr;
    DictDistilled r;
    if ((rc = dict_distill_records(node->eng[o], base->parts[o], base->blob_table, min_refs, flags,
                                   nullptr, o == 0 ? &keep : nullptr, true, &r, &p)))
      break;
    if (o == 0) res = r;
    if (o && (p->dev.m != d->parts[0]->dev.m || p->dev.n_blobs != d->parts[0]->dev.n_blobs)) {
      dict_unref(p);
      rc = fail(e0, NGPU_EINVAL, "node dict distill: the replicas differ");
      break;
    }
    d->parts.push_back(p);
  }
  if (!rc) {
    const uint64_t m = base->dev.m, s = res.s;
    d->dev.m = s;
    d->dev.n_blobs = res.plan.n_kept;
    // the global handle: placement rows only (if base keeps any), with a fork's room
    const DictPlace *rows = base->place();
    const uint64_t cap = dict_retire_rec_cap(s);
    if (!(rc = storage_alloc_place_only(e0, rows && s ? cap : 0, &d->st))) {
      d->st->rec_cap = cap;
      d->st->used = s;
      if (rows && s) {
        dict_retire_place(keep, m, rows, d->st->place, s);
        d->has_place = true;
      }
    }
  }
  if (rc) {
    dict_unref(d);
    return rc;
  }
  d->blob_table = dict_retire_blob_table(base->blob_table, res.plan.rows);
  *out = d;
  if (info) *info = res.info;
  return 0;
}

// ---- node dict retire across parts ---------------------------------------------
// ngpu_node_dict_retire_parts: the retire of a partitioned dict.  The parts tile
// the old global ids [0, m); a part's new global ids are ranks over all parts'
// keep bits.  Per part o, on a build stream on its device and one scratch
// allocation (node_retire_plan.hpp):
//   1. the retire bitmap and the remap go up, the part's bitmap over [0, m) is
//      zeroed, launch_node_keep_scan gives the local keep words, prefixes and s_o
//      and sets bit gid of every kept row; an event.  All W parts are enqueued
//      before anything waits.
//   2. the part's stream waits for every other part's event and copies their
//      bitmaps in (hipMemcpyPeerAsync; its own device to device);
//      launch_node_keep_merge ORs them, scans the popcounts and leaves s_o, S and
//      the three counters in one block, copied to pinned memory.  Part 0 also
//      brings the global keep words and prefixes back when base keeps placement
//      rows.  The same work on every part: no lead device, no broadcast, no
//      second exchange.  The call's only mid-way wait follows.
//   3. the host verdict; every refusal comes before a storage is allocated.
//   4. launch_node_dict_compact and launch_dict_build on every part's own new
//      storage, while the host compacts the node handle's placement rows by the
//      global keep words.
//   5. the handle, as the replicated path assembles it.
// Nothing of base's storages is written; every stream is waited for on every path.
struct RetirePart {
  std::unique_ptr<BuildStream> bs;
  hipEvent_t ready = nullptr;  // its bitmap is complete
  hipEvent_t t[6] = {};        // NGPU_DICT_TRACE=1: the ends of the call's device phases
  uint8_t *scr = nullptr;
  NodeRetireScratch lay;
  uint64_t m_o = 0;
  DictStorage *dst = nullptr;
};

// What node_dict_retire_parts and node_dict_distill_parts (below) share: the
// parts' streams, events and scratch, steps 2, 4 and 5 above, and the waits and
// releases of every path.  what: "node dict retire"; sym: the trace lines' name.
struct PartsCall {
  ngpu_node *node;
  ngpu_dict *base;
  const char *what, *sym;
  ngpu_engine *e0;
  const uint32_t W;
  const uint64_t m, gnw;
  const uint32_t nb0;
  const DictPlace *rows;
  bool trace;
  // the trace's host side: milliseconds since the call began at the end of each phase
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  double t_host[5] = {};
  std::vector<RetirePart> pt;
  // the engines' kept pinned counter words (fold_h, under fold_mu in index order as
  // node_dict_fold takes them): a pinned allocation per call costs milliseconds
  std::vector<std::unique_lock<std::mutex>> lanes;
  DictKeep keep;
  int rc = 0;

  PartsCall(ngpu_node *node_, ngpu_dict *base_, const char *what_, const char *sym_)
      : node(node_), base(base_), what(what_), sym(sym_), e0(node_->eng[0]),
        W((uint32_t)node_->eng.size()), m(base_->dev.m), gnw((base_->dev.m + 63) / 64),
        nb0(base_->dev.n_blobs), rows(base_->place()), pt(node_->eng.size()) {
    const char *tv = getenv("NGPU_DICT_TRACE");
    trace = tv && tv[0] == '1';
  }
  void stamp(int i) {
    if (trace)
      t_host[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  void mark(RetirePart &p, int i) {
    if (trace && p.t[i]) (void)hipEventRecord(p.t[i], p.bs->s);
  }
  int pinned() {
    for (uint32_t o = 0; o < W; ++o) lanes.emplace_back(node->eng[o]->fold_mu);
    for (uint32_t o = 0; o < W; ++o) {
      ngpu_engine *e = node->eng[o];
      DeviceGuard dg(e->device);
      if (!e->fold_h && hipHostMalloc((void **)&e->fold_h, 512) != hipSuccess) {
        (void)hipGetLastError();
        e->fold_h = nullptr;
        return fail(e0, NGPU_ENOMEM, "%s: pinned counters", what);
      }
    }
    return 0;
  }
  // Part o's stream, events (n_events of the trace's) and scratch of lay.bytes;
  // the caller holds a DeviceGuard of the part's device.  Sets rc on failure.
  bool part_begin(uint32_t o, const NodeRetireScratch &lay, int n_events) {
    RetirePart &p = pt[o];
    p.m_o = base->parts[o]->dev.m;
    p.lay = lay;
    p.bs.reset(new BuildStream(node->dev[o]));
    if (!p.bs->s || hipEventCreateWithFlags(&p.ready, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(e0, NGPU_EHIP, "%s: part %u: no build stream", what, o);
      return false;
    }
    for (int i = 0; trace && i < n_events; ++i)
      if (hipEventCreate(&p.t[i]) != hipSuccess) p.t[i] = nullptr;
    if (hipMalloc((void **)&p.scr, p.lay.bytes) != hipSuccess) {
      (void)hipGetLastError();
      p.scr = nullptr;
      rc = fail(e0, NGPU_ENOMEM, "%s: part %u: scratch allocation failed", what, o);
      return false;
    }
    return true;
  }
  void quiesce() {  // every stream the call used, whatever another one said
    for (uint32_t o = 0; o < W; ++o) {
      if (!pt[o].bs || !pt[o].bs->s) continue;
      DeviceGuard dg(node->dev[o]);
      if (hipStreamSynchronize(pt[o].bs->s) != hipSuccess && !rc)
        rc = fail(e0, NGPU_EHIP, "%s: part %u failed on its device", what, o);
    }
  }
  void release() {  // after quiesce(): the scratch, the events, storages not handed over
    for (uint32_t o = 0; o < W; ++o) {
      RetirePart &p = pt[o];
      DeviceGuard dg(node->dev[o]);
      if (p.scr) (void)hipFree(p.scr);
      p.scr = nullptr;
      if (p.ready) (void)hipEventDestroy(p.ready);
      p.ready = nullptr;
      for (hipEvent_t &ev : p.t) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
      }
      storage_unref(p.dst);
      p.dst = nullptr;
    }
  }
  // Step 2 on every part (rc == 0, every part's ready recorded): the all-gather of
  // the bitmaps, their OR and the global scan; ctr_words words from the part's
  // counter block go to its engine's pinned words, and part 0 brings the global
  // keep words and prefixes back when base keeps placement rows.  ev: the trace
  // event after the merge.
  void gather_merge(int ctr_words, int ev) {
    for (uint32_t o = 0; o < W && !rc; ++o) {
      RetirePart &p = pt[o];
      DeviceGuard dg(node->dev[o]);
      const hipStream_t s = p.bs->s;
      bool ok = true;
      for (uint32_t q = 0; q < W && ok && gnw; ++q) {
        uint8_t *to = p.scr + p.lay.gather + 8 * gnw * q;
        const uint8_t *from = pt[q].scr + pt[q].lay.own;
        if (q == o)  // written on this very stream
          ok = hipMemcpyAsync(to, from, 8 * gnw, hipMemcpyDeviceToDevice, s) == hipSuccess;
        else
          ok = hipStreamWaitEvent(s, pt[q].ready, 0) == hipSuccess &&
               hipMemcpyPeerAsync(to, node->dev[o], from, node->dev[q], 8 * gnw, s) == hipSuccess;
      }
      if (ok) {
        uint64_t *d_ctr = (uint64_t *)(p.scr + p.lay.ctr);
        launch_node_keep_merge((const uint64_t *)(p.scr + p.lay.gather), W, m,
                               (uint64_t *)(p.scr + p.lay.gwords), (uint32_t *)(p.scr + p.lay.gcnt),
                               (uint64_t *)(p.scr + p.lay.gsums),
                               (const uint64_t *)(p.scr + p.lay.sums) + dict_retire_scan_tiles(p.m_o), d_ctr,
                               s);
        mark(p, ev);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(node->eng[o]->fold_h, d_ctr, 8 * (size_t)ctr_words, hipMemcpyDeviceToHost, s) ==
                 hipSuccess;
      }
      if (ok && o == 0 && rows && gnw) {
        keep.words.resize(gnw);
        keep.prefix.resize(gnw);
        ok = hipMemcpyAsync(keep.words.data(), p.scr + p.lay.gwords, 8 * gnw, hipMemcpyDeviceToHost, s) ==
                 hipSuccess &&
             hipMemcpyAsync(keep.prefix.data(), p.scr + p.lay.gcnt, 4 * gnw, hipMemcpyDeviceToHost, s) ==
                 hipSuccess;
      }
      if (!ok) rc = fail(e0, NGPU_EHIP, "%s: part %u: gathering the keep bits failed", what, o);
    }
  }
  // Step 3's half that both calls have, after the mid-way wait: the retire
  // counters of every part (the first words of its pinned block) and their verdict.
  NodeRetireVerdict verdict() {
    std::vector<uint64_t> h_ctr((size_t)W * kNodeRetireCtrWords);
    for (uint32_t o = 0; o < W; ++o)
      memcpy(&h_ctr[(size_t)o * kNodeRetireCtrWords], node->eng[o]->fold_h, 8 * kNodeRetireCtrWords);
    const NodeRetireVerdict v = node_retire_verdict(W, h_ctr.data(), m);
    if (!v.ok())
      rc = fail(e0, NGPU_EINVAL,
                "%s: the parts do not tile the dict's ids (%s, part %u; %llu survivors of %llu)", what,
                v.refusal == kNodeRetireCounter
                    ? (v.which == kNodeRetireBadGid ? "an id past the dict's entries"
                       : v.which == kNodeRetireDupBit ? "an id held twice" : "an id held by two parts")
                    : v.refusal == kNodeRetireSum ? "the parts' survivors do not add up" : "too many survivors",
                v.bad, (unsigned long long)v.S, (unsigned long long)m);
    return v;
  }
  // Steps 4 and 5 (rc == 0, the remap of nb0 words in every part's scratch, or
  // ordered before this on its stream): every part's survivors onto a storage of
  // its own and its table, the node handle's placement rows meanwhile, the last
  // wait and the handle of n_kept blobs, its blob table base's rows by blob_rows.
  // ev: the trace events around the compaction are ev and ev + 1; part_line(o, p):
  // the part's trace line.  Releases everything on every path.
  template <class Line>
  int finish(const NodeRetireVerdict &v, uint32_t n_kept, const std::vector<uint32_t> &blob_rows, int ev,
             Line &&part_line, ngpu_dict **out) {
    const NodeRetireCaps caps = node_retire_caps(v);
    const uint64_t S = v.S;
    for (uint32_t o = 0; o < W && !rc; ++o) {
      RetirePart &p = pt[o];
      const ngpu_dict *bp = base->parts[o];
      DeviceGuard dg(node->dev[o]);
      if ((rc = storage_alloc(node->eng[o], caps.rec_cap[o], caps.table_cap[o], false, &p.dst))) {
        rc = fail(e0, rc, "%s", ngpu_last_error(node->eng[o]));
        break;
      }
      p.dst->used = v.s[o];
      const hipStream_t s = p.bs->s;
      mark(p, ev);
      launch_node_dict_compact(bp->st ? bp->st->rec : nullptr, p.m_o, (const uint64_t *)(p.scr + p.lay.words),
                               (const uint32_t *)(p.scr + p.lay.cnt), (const uint64_t *)(p.scr + p.lay.gwords),
                               (const uint32_t *)(p.scr + p.lay.gcnt), m, (const uint32_t *)(p.scr + p.lay.remap),
                               nb0, p.dst->rec, v.s[o], s);
      launch_dict_build(p.dst->rec, v.s[o], p.dst->table, p.dst->table_cap, s);
      mark(p, ev + 1);
      if (hipGetLastError() != hipSuccess)
        rc = fail(e0, NGPU_EHIP, "%s: part %u: compaction failed", what, o);
    }
    stamp(2);
    // the node handle's placement rows, while the devices move the records
    DictStorage *hst = nullptr;
    if (!rc && !(rc = storage_alloc_place_only(e0, rows && S ? caps.place_cap : 0, &hst))) {
      hst->rec_cap = caps.place_cap;
      hst->used = S;
      if (rows && S) dict_retire_place(keep, m, rows, hst->place, S);
    }
    quiesce();
    stamp(3);
    if (rc) {
      storage_unref(hst);
      release();
      return rc;
    }
    if (trace)
      for (uint32_t o = 0; o < W; ++o) {
        part_line(o, pt[o]);
        (void)hipGetLastError();
      }
    ngpu_dict *d = dict_derive(base);
    d->dev.m = S;
    d->dev.n_blobs = n_kept;
    d->st = hst;
    d->has_place = rows && S;
    for (uint32_t o = 0; o < W; ++o) {
      ngpu_dict *p = dict_derive(base->parts[o]);
      p->st = pt[o].dst;
      pt[o].dst = nullptr;
      dict_bind(p, v.s[o], n_kept);
      d->parts.push_back(p);
    }
    d->blob_table = dict_retire_blob_table(base->blob_table, blob_rows);
    release();
    stamp(4);
    if (trace)
      fprintf(stderr,
              "ngpu %s host W=%u m=%llu enqueue_ms=%.3f wait_ms=%.3f alloc_launch_ms=%.3f "
              "place_wait_ms=%.3f release_ms=%.3f\n",
              sym, W, (unsigned long long)m, t_host[0], t_host[1] - t_host[0], t_host[2] - t_host[1],
              t_host[3] - t_host[2], t_host[4] - t_host[3]);
    *out = d;
    return 0;
  }
};

// The device time between two of a part's trace events, in microseconds (-1: none).
double part_us(const RetirePart &p, int a, int b) {
  float ms = 0;
  if (!p.t[a] || !p.t[b] || hipEventElapsedTime(&ms, p.t[a], p.t[b]) != hipSuccess) return -1.0;
  return ms * 1000.0;
}

int node_dict_retire_parts(ngpu_node *node, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                           ngpu_dict **out) {
  ngpu_engine *e0 = node->eng[0];
  if (int rc = node_dict_base_check(node, base, "retire")) return rc;
  if (base->replicated) return node_dict_retire(node, base, blobs, n, out);
  const DictRetirePlan plan = dict_retire_plan(base->dev.n_blobs, blobs, n);
  if (!plan.ok)
    return fail(e0, NGPU_EINVAL, "node dict retire: blob %u of a dict of %u blobs", plan.bad,
                base->dev.n_blobs);
  PartsCall c(node, base, "node dict retire", "node_dict_retire_parts");
  const uint32_t W = c.W;
  const uint64_t m = c.m, gnw = c.gnw;
  if (int rc = c.pinned()) return rc;
  static_assert(8 * kNodeRetireCtrWords <= 512, "the counters fit the engines' pinned words");

  // 1. every part's keep words and its bitmap over the global ids
  for (uint32_t o = 0; o < W && !c.rc; ++o) {
    const ngpu_dict *bp = base->parts[o];
    DeviceGuard dg(node->dev[o]);
    if (!c.part_begin(o, node_retire_scratch_layout(bp->dev.m, m, W, plan.bitmap.size(), plan.remap.size()),
                      5))
      break;
    RetirePart &p = c.pt[o];
    const hipStream_t s = p.bs->s;
    uint64_t *d_ctr = (uint64_t *)(p.scr + p.lay.ctr);
    bool ok = hipMemcpyAsync(p.scr + p.lay.bits, plan.bitmap.data(), 4 * plan.bitmap.size(),
                             hipMemcpyHostToDevice, s) == hipSuccess &&
              (plan.remap.empty() || hipMemcpyAsync(p.scr + p.lay.remap, plan.remap.data(),
                                                    4 * plan.remap.size(), hipMemcpyHostToDevice,
                                                    s) == hipSuccess) &&
              hipMemsetAsync(d_ctr, 0, 8 * kNodeRetireCtrWords, s) == hipSuccess &&
              (!gnw || hipMemsetAsync(p.scr + p.lay.own, 0, 8 * gnw, s) == hipSuccess);
    if (ok) {
      c.mark(p, 0);
      launch_node_keep_scan(bp->st ? bp->st->rec : nullptr, p.m_o, (const uint32_t *)(p.scr + p.lay.bits),
                            c.nb0, m, (uint64_t *)(p.scr + p.lay.words), (uint32_t *)(p.scr + p.lay.cnt),
                            (uint64_t *)(p.scr + p.lay.sums), (uint64_t *)(p.scr + p.lay.own), d_ctr, s);
      c.mark(p, 1);
      ok = hipGetLastError() == hipSuccess && hipEventRecord(p.ready, s) == hipSuccess;
    }
    if (!ok) c.rc = fail(e0, NGPU_EHIP, "node dict retire: part %u: keep scan failed", o);
  }
  // 2. all-gather of the bitmaps, their OR and the global scan, on every part
  c.gather_merge(kNodeRetireCtrWords, 2);
  c.stamp(0);
  c.quiesce();  // the call's only mid-way wait
  c.stamp(1);
  if (c.rc) {
    c.release();
    return c.rc;
  }
  // 3. the verdict; nothing is allocated before it
  const NodeRetireVerdict v = c.verdict();
  if (c.rc) {
    c.release();
    return c.rc;
  }
  // 4. and 5.
  return c.finish(v, plan.n_kept, plan.remap, 3,
                  [&](uint32_t o, const RetirePart &p) {
                    const double a = part_us(p, 0, 1), b = part_us(p, 1, 2), k = part_us(p, 3, 4);
                    if (a >= 0 && b >= 0 && k >= 0)
                      fprintf(stderr,
                              "ngpu node_dict_retire_parts part=%u m=%llu m_o=%llu s_o=%llu device_us=%.1f "
                              "keep_scan_us=%.1f gather_merge_us=%.1f compact_build_us=%.1f\n",
                              o, (unsigned long long)m, (unsigned long long)p.m_o, (unsigned long long)v.s[o],
                              a + b + k, a, b, k);
                  },
                  out);
}

// ---- node dict distill across parts --------------------------------------------
// ngpu_node_dict_distill_parts: the distill of a partitioned dict.  All rows of a
// digest live on one part and a part's rows are in ascending gid order, so a part
// counts its own rows through its own table and its winners are the dict's; the
// survivors' new global ids and the live blobs are over all parts.  The steps are
// those of node_dict_retire_parts above, with these differences:
//   1. refs, the counters (a retire's and distill's 35, side by side), the live
//      words and the part's bitmap are zeroed; launch_dict_ref_count, then
//      launch_node_distill_keep_scan (node_distill.hip): distill's keep pass and
//      the retire's in one.
//   2. the same exchange; the one copy of counters brings both blocks back, a
//      second the part's live bitmap (to memory of the call's own).
//   3. the verdict, then node_distill_sum (node_distill_plan.hpp): every part's
//      counters against its m_o and s_o, their sums, the OR of the live bitmaps;
//      distill_blob_plan over the union; the remap goes up to every part.  A
//      count-only call ends here.
//   4. and 5. unchanged.
int node_dict_distill_parts(ngpu_node *node, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                            ngpu_dict **out, ngpu_dict_distill_info *info) {
  ngpu_engine *e0 = node->eng[0];
  if (int rc = node_dict_base_check(node, base, "distill")) return rc;
  if ((flags & NGPU_DICT_DISTILL_MERGE_BLOB_IDS) && base->dev.m && base->blob_table.empty())
    return fail(e0, NGPU_EINVAL,
                "node dict distill: blob ids are merged by the blob table, the dict has none");
  if (base->replicated) return node_dict_distill(node, base, min_refs, flags, out, info);
  if (base->dev.n_blobs > kDictMaxBlobs)
    return fail(e0, NGPU_EINVAL, "node dict distill: a dict of %u blobs", base->dev.n_blobs);
  PartsCall c(node, base, "node dict distill", "node_dict_distill_parts");
  const uint32_t W = c.W, nb0 = c.nb0;
  const uint64_t m = c.m, gnw = c.gnw, lw = distill_live_words(nb0);
  std::vector<uint64_t> m_o(W);
  uint64_t total = 0;
  for (uint32_t o = 0; o < W; ++o) total += m_o[o] = base->parts[o]->dev.m;
  if (total != m)
    return fail(e0, NGPU_EINVAL, "node dict distill: the parts hold %llu rows, the dict %llu entries",
                (unsigned long long)total, (unsigned long long)m);
  if (int rc = c.pinned()) return rc;
  static_assert(8 * kNodeDistillBackWords <= 512, "the counters fit the engines' pinned words");
  std::vector<uint32_t> h_live((size_t)W * lw, 0);
  std::vector<NodeDistillScratch> lay(W);

  // 1. every part's counts, keep words and its bitmap over the global ids
  for (uint32_t o = 0; o < W && !c.rc; ++o) {
    const ngpu_dict *bp = base->parts[o];
    DeviceGuard dg(node->dev[o]);
    lay[o] = node_distill_scratch_layout(m_o[o], m, W, nb0);
    if (!c.part_begin(o, lay[o].r, 6)) break;
    RetirePart &p = c.pt[o];
    const hipStream_t s = p.bs->s;
    uint64_t *d_ctr = (uint64_t *)(p.scr + p.lay.ctr);
    uint32_t *d_refs = (uint32_t *)(p.scr + lay[o].refs);
    const DictRec *rec = bp->st ? bp->st->rec : nullptr;
    bool ok = hipMemsetAsync(d_ctr, 0, 8 * kNodeDistillBackWords, s) == hipSuccess &&
              hipMemsetAsync(p.scr + lay[o].live, 0, lay[o].zero_bytes, s) == hipSuccess &&
              (!gnw || hipMemsetAsync(p.scr + p.lay.own, 0, 8 * gnw, s) == hipSuccess);
    if (ok) {
      c.mark(p, 0);
      launch_dict_ref_count(rec, p.m_o, bp->st ? bp->st->table : nullptr, bp->st ? bp->st->table_cap : 0,
                            d_refs, s);
      c.mark(p, 1);
      launch_node_distill_keep_scan(rec, p.m_o, d_refs, min_refs, nb0, m, (uint64_t *)(p.scr + p.lay.words),
                                    (uint32_t *)(p.scr + p.lay.cnt), (uint64_t *)(p.scr + p.lay.sums),
                                    (uint32_t *)(p.scr + lay[o].live), (uint64_t *)(p.scr + lay[o].stats),
                                    (uint64_t *)(p.scr + p.lay.own), d_ctr, s);
      c.mark(p, 2);
      ok = hipGetLastError() == hipSuccess && hipEventRecord(p.ready, s) == hipSuccess;
    }
    if (!ok) c.rc = fail(e0, NGPU_EHIP, "node dict distill: part %u: counting failed", o);
  }
  // 2. all-gather of the bitmaps, their OR and the global scan, on every part;
  //    the counters and the live blobs come back
  c.gather_merge(kNodeDistillBackWords, 3);
  for (uint32_t o = 0; o < W && !c.rc; ++o) {
    DeviceGuard dg(node->dev[o]);
    if (hipMemcpyAsync(&h_live[(size_t)o * lw], c.pt[o].scr + lay[o].live, 4 * lw, hipMemcpyDeviceToHost,
                       c.pt[o].bs->s) != hipSuccess)
      c.rc = fail(e0, NGPU_EHIP, "node dict distill: part %u: the live blobs did not come back", o);
  }
  c.stamp(0);
  c.quiesce();  // the call's only mid-way wait
  c.stamp(1);
  if (c.rc) {
    c.release();
    return c.rc;
  }
  // 3. the verdict, the counters of the whole dict and what becomes of the blobs;
  //    nothing is allocated before it
  const NodeRetireVerdict v = c.verdict();
  if (c.rc) {
    c.release();
    return c.rc;
  }
  std::vector<uint64_t> h_back((size_t)W * kNodeDistillBackWords);
  for (uint32_t o = 0; o < W; ++o)
    memcpy(&h_back[(size_t)o * kNodeDistillBackWords], node->eng[o]->fold_h, 8 * kNodeDistillBackWords);
  const NodeDistillSum sum = node_distill_sum(W, h_back.data(), h_live.data(), nb0, m_o.data(), v.s.data());
  if (!sum.ok(W)) {
    const uint64_t *st = &h_back[(size_t)sum.bad_part * kNodeDistillBackWords + kNodeRetireCtrWords];
    c.rc = fail(e0, NGPU_EHIP, "node dict distill: part %u: %llu survivors, %llu digests of %llu records",
                sum.bad_part, (unsigned long long)v.s[sum.bad_part], (unsigned long long)st[kDistillDistinct],
                (unsigned long long)m_o[sum.bad_part]);
    c.release();
    return c.rc;
  }
  const DistillBlobPlan plan = distill_blob_plan(
      nb0, sum.live.data(), flags,
      base->blob_table.size() >= 256ull * nb0 && nb0 ? base->blob_table.data() : nullptr);
  if (!plan.ok) {
    c.rc = fail(e0, NGPU_EINVAL, "node dict distill: a dict of %u blobs", nb0);
    c.release();
    return c.rc;
  }
  if (info) distill_info_fill(info, m, sum.stats, nb0, plan.n_kept);
  if (!out) {  // a count
    if (c.trace)
      for (uint32_t o = 0; o < W; ++o) {
        const RetirePart &p = c.pt[o];
        const double a = part_us(p, 0, 1), b = part_us(p, 1, 2), g = part_us(p, 2, 3);
        if (a >= 0 && b >= 0 && g >= 0)
          fprintf(stderr,
                  "ngpu node_dict_distill_parts part=%u m=%llu m_o=%llu s_o=%llu device_us=%.1f count_us=%.1f "
                  "keep_scan_us=%.1f gather_merge_us=%.1f compact_build_us=%.1f\n",
                  o, (unsigned long long)m, (unsigned long long)p.m_o, (unsigned long long)v.s[o], a + b + g, a,
                  b, g, 0.0);
        (void)hipGetLastError();
      }
    c.release();
    return 0;
  }
  for (uint32_t o = 0; o < W && !c.rc && nb0; ++o) {
    DeviceGuard dg(node->dev[o]);
    if (hipMemcpyAsync(c.pt[o].scr + c.pt[o].lay.remap, plan.remap.data(), 4ull * nb0, hipMemcpyHostToDevice,
                       c.pt[o].bs->s) != hipSuccess)
      c.rc = fail(e0, NGPU_EHIP, "node dict distill: part %u: upload failed", o);
  }
  if (c.rc) {
    c.quiesce();
    c.release();
    return c.rc;
  }
  // 4. and 5.
  return c.finish(v, plan.n_kept, plan.rows, 4,
                  [&](uint32_t o, const RetirePart &p) {
                    const double a = part_us(p, 0, 1), b = part_us(p, 1, 2), g = part_us(p, 2, 3),
                                 k = part_us(p, 4, 5);
                    if (a >= 0 && b >= 0 && g >= 0 && k >= 0)
                      fprintf(stderr,
                              "ngpu node_dict_distill_parts part=%u m=%llu m_o=%llu s_o=%llu device_us=%.1f "
                              "count_us=%.1f keep_scan_us=%.1f gather_merge_us=%.1f compact_build_us=%.1f\n",
                              o, (unsigned long long)m, (unsigned long long)p.m_o, (unsigned long long)v.s[o],
                              a + b + g + k, a, b, g, k);
                  },
                  out);
}

// ---- node dict remode ----------------------------------------------------------
// ngpu_node_dict_remode: base's rows in the other mode, moved on the GPUs.  The
// rows, their global ids and blobs, the blob table and the node handle's placement
// rows are base's; only where the rows live differs.  The parts' streams, events,
// scratch, waits and releases are PartsCall's, the host plan node_remode_plan.hpp,
// the kernels node_remode.hip.
//   split (replicated -> partitioned), part o on the replica of its own device:
//     1. launch_remode_split_keep_scan: keep = the part owns the row's digest, the
//        scan; s_o comes back in one 8-B copy.  All W parts are enqueued before the
//        call's one mid-way wait.
//     2. the verdict: sum s_o == m; nothing is allocated before it.
//     3. launch_remode_split_compact and launch_dict_build on the part's new storage.
//   join (partitioned -> replicated):
//     1. every part's rows at every window cut (launch_node_save_bounds), one launch
//        and one copy back per part; the one mid-way wait; the slices' verdict, which
//        bounds every copy below.
//     2. replica j, on a storage for all m rows: per window the other parts' slices
//        are peer-copied into one of two staging windows on a copy stream while the
//        main stream scatters j's own slice and the window before; then the bitmap's
//        count, the counters' copy back and launch_dict_build over the m rows.
//     3. the verdict after the last wait; a refusal frees everything.
//   same mode: ngpu_node_dict_retire_parts' compacting copy (n == 0) with the
//   exchange the target asks for.
// Nothing of base's storages is written; every stream is waited for on every path.

// The node handle's storage of a remode: base's placement rows (if it keeps any)
// with a fork's room.
int remode_place(PartsCall &c, DictStorage **hst) {
  const uint64_t cap = remode_caps(c.m).rec_cap;
  if (int rc = storage_alloc_place_only(c.e0, c.rows && c.m ? cap : 0, hst)) return rc;
  (*hst)->rec_cap = cap;
  (*hst)->used = c.m;
  if (c.rows && c.m) memcpy((*hst)->place, c.rows, c.m * sizeof(DictPlace));
  return 0;
}

// The handle over the parts' new storages (pt[o].dst, s[o] rows each), handed over.
ngpu_dict *remode_handle(PartsCall &c, const std::vector<uint64_t> &s, DictStorage *hst, bool replicated,
                         bool routed) {
  ngpu_dict *d = dict_derive(c.base);
  d->replicated = replicated;
  d->routed = routed;
  d->dev.m = c.m;
  d->dev.n_blobs = c.nb0;
  d->st = hst;
  d->has_place = c.rows && c.m;
  for (uint32_t o = 0; o < c.W; ++o) {
    ngpu_dict *p = dict_derive(c.base->parts[o]);
    p->st = c.pt[o].dst;
    c.pt[o].dst = nullptr;
    dict_bind(p, s[o], c.nb0);
    d->parts.push_back(p);
  }
  d->blob_table = c.base->blob_table;
  return d;
}

NodeRetireScratch remode_scratch_bytes(uint64_t bytes) {  // (PartsCall allocates lay.bytes)
  NodeRetireScratch r;
  r.bytes = bytes;
  return r;
}

int node_dict_split(ngpu_node *node, ngpu_dict *base, bool routed, ngpu_dict **out) {
  PartsCall c(node, base, "node dict remode", "node_dict_remode");
  ngpu_engine *e0 = c.e0;
  const uint32_t W = c.W;
  const uint64_t m = c.m;
  for (uint32_t o = 0; o < W; ++o)
    if (base->parts[o]->dev.m != m)
      return fail(e0, NGPU_EINVAL, "node dict remode: replica %u of %llu entries, dict of %llu", o,
                  (unsigned long long)base->parts[o]->dev.m, (unsigned long long)m);
  if (int rc = c.pinned()) return rc;
  const RemodeSplitScratch lay = remode_split_scratch_layout(m);

  // 1. every part's keep words, prefixes and s_o
  for (uint32_t o = 0; o < W && !c.rc; ++o) {
    const ngpu_dict *bp = base->parts[o];
    DeviceGuard dg(node->dev[o]);
    if (!c.part_begin(o, remode_scratch_bytes(lay.bytes), 4)) break;
    RetirePart &p = c.pt[o];
    const hipStream_t s = p.bs->s;
    c.mark(p, 0);
    launch_remode_split_keep_scan(bp->st ? bp->st->rec : nullptr, m, W, o, (uint64_t *)(p.scr + lay.words),
                                  (uint32_t *)(p.scr + lay.cnt), (uint64_t *)(p.scr + lay.sums), s);
    c.mark(p, 1);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(node->eng[o]->fold_h, p.scr + remode_split_total_at(lay, m), 8, hipMemcpyDeviceToHost,
                       s) != hipSuccess)
      c.rc = fail(e0, NGPU_EHIP, "node dict remode: part %u: keep scan failed", o);
  }
  c.stamp(0);
  c.quiesce();  // the call's only mid-way wait
  c.stamp(1);
  // 2. the verdict; nothing is allocated before it
  std::vector<uint64_t> s_o(W, 0);
  if (!c.rc) {
    for (uint32_t o = 0; o < W; ++o) s_o[o] = node->eng[o]->fold_h[0];
    const RemodeVerdict v = remode_split_verdict(W, s_o.data(), m);
    if (!v.ok())
      c.rc = fail(e0, NGPU_EINVAL, "node dict remode: %s (%llu of %llu)", remode_refusal(v.refusal),
                  (unsigned long long)v.got, (unsigned long long)v.want);
  }
  if (c.rc) {
    c.release();
    return c.rc;
  }
  // 3. every part's rows onto a storage of its own, and its table
  for (uint32_t o = 0; o < W && !c.rc; ++o) {
    RetirePart &p = c.pt[o];
    const ngpu_dict *bp = base->parts[o];
    DeviceGuard dg(node->dev[o]);
    const RemodeCaps caps = remode_caps(s_o[o]);
    if ((c.rc = storage_alloc(node->eng[o], caps.rec_cap, caps.table_cap, false, &p.dst))) {
      c.rc = fail(e0, c.rc, "%s", ngpu_last_error(node->eng[o]));
      break;
    }
    p.dst->used = s_o[o];
    const hipStream_t s = p.bs->s;
    c.mark(p, 2);
    launch_remode_split_compact(bp->st ? bp->st->rec : nullptr, m, (const uint64_t *)(p.scr + lay.words),
                                (const uint32_t *)(p.scr + lay.cnt), p.dst->rec, s_o[o], s);
    launch_dict_build(p.dst->rec, s_o[o], p.dst->table, p.dst->table_cap, s);
    c.mark(p, 3);
    if (hipGetLastError() != hipSuccess)
      c.rc = fail(e0, NGPU_EHIP, "node dict remode: part %u: compaction failed", o);
  }
  c.stamp(2);
  DictStorage *hst = nullptr;  // the node handle's rows, while the devices move the records
  if (!c.rc) c.rc = remode_place(c, &hst);
  c.quiesce();
  c.stamp(3);
  if (c.rc) {
    storage_unref(hst);
    c.release();
    return c.rc;
  }
  if (c.trace)
    for (uint32_t o = 0; o < W; ++o) {
      const RetirePart &p = c.pt[o];
      const double a = part_us(p, 0, 1), k = part_us(p, 2, 3);
      if (a >= 0 && k >= 0)
        fprintf(stderr,
                "ngpu node_dict_remode split part=%u m=%llu s_o=%llu device_us=%.1f keep_scan_us=%.1f "
                "compact_build_us=%.1f\n",
                o, (unsigned long long)m, (unsigned long long)s_o[o], a + k, a, k);
      (void)hipGetLastError();
    }
  ngpu_dict *d = remode_handle(c, s_o, hst, false, routed);
  c.release();
  c.stamp(4);
  if (c.trace)
    fprintf(stderr,
            "ngpu node_dict_remode split host W=%u m=%llu enqueue_ms=%.3f wait_ms=%.3f alloc_launch_ms=%.3f "
            "place_wait_ms=%.3f release_ms=%.3f\n",
            W, (unsigned long long)m, c.t_host[0], c.t_host[1] - c.t_host[0], c.t_host[2] - c.t_host[1],
            c.t_host[3] - c.t_host[2], c.t_host[4] - c.t_host[3]);
  *out = d;
  return 0;
}

// A replica's copy stream and the events of its two staging windows (join).
struct JoinSide {
  std::unique_ptr<BuildStream> cs;
  hipEvent_t copied[2] = {}, scattered[2] = {};
  bool used[2] = {false, false};
};

int node_dict_join(ngpu_node *node, ngpu_dict *base, uint64_t window_records, ngpu_dict **out) {
  PartsCall c(node, base, "node dict remode", "node_dict_remode");
  ngpu_engine *e0 = c.e0;
  const uint32_t W = c.W;
  const uint64_t m = c.m;
  std::vector<uint64_t> m_o(W);
  uint64_t total = 0;
  for (uint32_t o = 0; o < W; ++o) total += m_o[o] = base->parts[o]->dev.m;
  if (total != m)
    return fail(e0, NGPU_EINVAL, "node dict remode: the parts hold %llu rows, the dict %llu entries",
                (unsigned long long)total, (unsigned long long)m);
  const uint64_t cw = remode_window_records(window_records, m), nw = remode_windows(m, cw);
  if (int rc = c.pinned()) return rc;
  static_assert(8 * kRemodeCtrWords <= 512, "the counters fit the engines' pinned words");
  const RemodeJoinScratch lay = remode_join_scratch_layout(m, cw);
  std::vector<std::vector<uint64_t>> off(W, std::vector<uint64_t>(nw + 1, 0));
  std::vector<JoinSide> side(W);
  auto rec_of = [&](uint32_t o) { return base->parts[o]->st ? base->parts[o]->st->rec : (const DictRec *)nullptr; };
  auto quiesce = [&] {  // the copy streams too
    c.quiesce();
    for (uint32_t j = 0; j < W; ++j) {
      if (!side[j].cs || !side[j].cs->s) continue;
      DeviceGuard dg(node->dev[j]);
      if (hipStreamSynchronize(side[j].cs->s) != hipSuccess && !c.rc)
        c.rc = fail(e0, NGPU_EHIP, "node dict remode: replica %u: its copies failed", j);
    }
  };
  auto release = [&] {  // after quiesce()
    for (uint32_t j = 0; j < W; ++j) {
      DeviceGuard dg(node->dev[j]);
      for (int k = 0; k < 2; ++k) {
        if (side[j].copied[k]) (void)hipEventDestroy(side[j].copied[k]);
        if (side[j].scattered[k]) (void)hipEventDestroy(side[j].scattered[k]);
      }
      side[j].cs.reset();
    }
    c.release();
  };

  // 1. every part's rows at every cut
  for (uint32_t o = 0; o < W && !c.rc; ++o) {
    DeviceGuard dg(node->dev[o]);
    if (!c.part_begin(o, remode_scratch_bytes(lay.bytes), 6)) break;
    RetirePart &p = c.pt[o];
    const hipStream_t s = p.bs->s;
    c.mark(p, 0);
    launch_node_save_bounds(rec_of(o), m_o[o], 0, m, cw, nw, (uint64_t *)(p.scr + lay.off), s);
    c.mark(p, 1);
    // (off's pageable memory: the stream is synchronised before it is read or freed)
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(off[o].data(), p.scr + lay.off, 8 * (nw + 1), hipMemcpyDeviceToHost, s) != hipSuccess)
      c.rc = fail(e0, NGPU_EHIP, "node dict remode: part %u: the window cuts failed", o);
  }
  c.stamp(0);
  c.quiesce();  // the call's only mid-way wait
  c.stamp(1);
  if (!c.rc) {  // no copy below leaves a part or overruns a staging window
    const RemodeVerdict v = remode_join_slices(W, m, cw, off, m_o.data());
    if (!v.ok())
      c.rc = fail(e0, NGPU_EINVAL,
                  "node dict remode: the parts do not tile the dict's ids (%s: part %u, window %llu, %llu of %llu)",
                  remode_refusal(v.refusal), v.bad, (unsigned long long)v.window, (unsigned long long)v.got,
                  (unsigned long long)v.want);
  }
  if (c.rc) {
    release();
    return c.rc;
  }
  // 2. every replica: its storage, the windows, the counters, its table
  const RemodeCaps caps = remode_caps(m);
  for (uint32_t j = 0; j < W && !c.rc; ++j) {
    RetirePart &p = c.pt[j];
    JoinSide &sd = side[j];
    DeviceGuard dg(node->dev[j]);
    if ((c.rc = storage_alloc(node->eng[j], caps.rec_cap, caps.table_cap, false, &p.dst))) {
      c.rc = fail(e0, c.rc, "%s", ngpu_last_error(node->eng[j]));
      break;
    }
    p.dst->used = m;
    sd.cs.reset(new BuildStream(node->dev[j]));
    bool ok = sd.cs->s != nullptr;
    for (int k = 0; k < 2 && ok; ++k)
      ok = hipEventCreateWithFlags(&sd.copied[k], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&sd.scattered[k], hipEventDisableTiming) == hipSuccess;
    const hipStream_t s = p.bs->s, cs = sd.cs->s;
    uint64_t *d_bits = (uint64_t *)(p.scr + lay.bits), *d_ctr = (uint64_t *)(p.scr + lay.ctr);
    // (the bitmap and the counters lie back to back)
    ok = ok && hipMemsetAsync(d_bits, 0, lay.off - lay.bits, s) == hipSuccess;
    c.mark(p, 2);
    for (uint64_t t = 0; t < nw && ok; ++t) {
      const int slot = (int)(t & 1);
      const uint64_t a = remode_cut(m, cw, t), n = remode_cut(m, cw, t + 1) - a;
      DictRec *stage = (DictRec *)(p.scr + lay.stage[slot]);
      uint64_t staged = 0;
      for (uint32_t q = 0; q < W && ok; ++q) {
        const uint64_t cnt = off[q][t + 1] - off[q][t];
        if (q == j || !cnt) continue;
        // the window before last has left this staging window
        if (!staged && sd.used[slot]) ok = hipStreamWaitEvent(cs, sd.scattered[slot], 0) == hipSuccess;
        ok = ok && hipMemcpyPeerAsync(stage + staged, node->dev[j], rec_of(q) + off[q][t], node->dev[q],
                                      cnt * sizeof(DictRec), cs) == hipSuccess;
        staged += cnt;  // (<= n <= cw: remode_join_slices)
      }
      if (staged) ok = ok && hipEventRecord(sd.copied[slot], cs) == hipSuccess;
      // j's own slice is read where it lies, while the copies run
      const uint64_t own = off[j][t + 1] - off[j][t];
      if (ok && own) launch_remode_join_scatter(rec_of(j) + off[j][t], own, a, n, m, p.dst->rec, d_bits, d_ctr, s);
      if (ok && staged) {
        ok = hipStreamWaitEvent(s, sd.copied[slot], 0) == hipSuccess;
        if (ok) launch_remode_join_scatter(stage, staged, a, n, m, p.dst->rec, d_bits, d_ctr, s);
        ok = ok && hipEventRecord(sd.scattered[slot], s) == hipSuccess;
        sd.used[slot] = true;
      }
    }
    if (ok) {
      launch_remode_bitmap_count(d_bits, m, d_ctr, s);
      c.mark(p, 3);
      ok = hipGetLastError() == hipSuccess &&
           hipMemcpyAsync(node->eng[j]->fold_h, d_ctr, 8 * kRemodeCtrWords, hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (ok) {
      // (a refused call builds over rows never written: the table is bounded by its
      // capacity whatever they hold, and it is freed with the storage)
      c.mark(p, 4);
      launch_dict_build(p.dst->rec, m, p.dst->table, p.dst->table_cap, s);
      c.mark(p, 5);
      ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) {
      (void)hipGetLastError();
      c.rc = fail(e0, NGPU_EHIP, "node dict remode: replica %u: moving its rows failed", j);
    }
  }
  c.stamp(2);
  DictStorage *hst = nullptr;  // the node handle's rows, while the devices move the records
  if (!c.rc) c.rc = remode_place(c, &hst);
  quiesce();
  c.stamp(3);
  // 3. the verdict
  if (!c.rc) {
    std::vector<uint64_t> h_ctr((size_t)W * kRemodeCtrWords);
    for (uint32_t j = 0; j < W; ++j)
      memcpy(&h_ctr[(size_t)j * kRemodeCtrWords], node->eng[j]->fold_h, 8 * kRemodeCtrWords);
    const RemodeVerdict v = remode_join_verdict(W, h_ctr.data(), m);
    if (!v.ok())
      c.rc = fail(e0, NGPU_EINVAL,
                  "node dict remode: the parts do not tile the dict's ids (%s: replica %u, %llu, %llu entries)",
                  remode_refusal(v.refusal), v.bad, (unsigned long long)v.got, (unsigned long long)m);
  }
  if (c.rc) {
    storage_unref(hst);
    release();
    return c.rc;
  }
  if (c.trace)
    for (uint32_t o = 0; o < W; ++o) {
      const RetirePart &p = c.pt[o];
      const double a = part_us(p, 0, 1), b = part_us(p, 2, 3), k = part_us(p, 4, 5);
      if (a >= 0 && b >= 0 && k >= 0)
        fprintf(stderr,
                "ngpu node_dict_remode join part=%u m=%llu m_o=%llu windows=%llu device_us=%.1f bounds_us=%.1f "
                "copy_scatter_us=%.1f build_us=%.1f\n",
                o, (unsigned long long)m, (unsigned long long)m_o[o], (unsigned long long)nw, a + b + k, a, b, k);
      (void)hipGetLastError();
    }
  ngpu_dict *d = remode_handle(c, std::vector<uint64_t>(W, m), hst, true, false);
  release();
  c.stamp(4);
  if (c.trace)
    fprintf(stderr,
            "ngpu node_dict_remode join host W=%u m=%llu enqueue_ms=%.3f wait_ms=%.3f alloc_launch_ms=%.3f "
            "place_wait_ms=%.3f release_ms=%.3f\n",
            W, (unsigned long long)m, c.t_host[0], c.t_host[1] - c.t_host[0], c.t_host[2] - c.t_host[1],
            c.t_host[3] - c.t_host[2], c.t_host[4] - c.t_host[3]);
  *out = d;
  return 0;
}

int node_dict_remode(ngpu_node *node, ngpu_dict *base, uint32_t mode, uint64_t window_records,
                     ngpu_dict **out) {
  bool replicated = false, routed = false;
  if (int rc = node_dict_mode(node, mode, &replicated, &routed)) return rc;
  if (base->parts.empty())
    return fail(node->eng[0], NGPU_EINVAL, "node dict remode: not a node dict (a plain dict has no mode)");
  if (int rc = node_dict_base_check(node, base, "remode")) return rc;
  if (replicated == base->replicated) {  // the compacting copy, with the exchange asked for
    ngpu_dict *d = nullptr;
    if (int rc = node_dict_retire_parts(node, base, nullptr, 0, &d)) return rc;
    d->routed = routed;
    *out = d;
    return 0;
  }
  return replicated ? node_dict_join(node, base, window_records, out)
                    : node_dict_split(node, base, routed, out);
}

// ngpu_node_dict_export of a partitioned dict: every part's HBM rows come back in
// pieces of 1M and each becomes the record at position gid, with the node
// handle's placement row gid.  The host checks that the parts tile [0, m): every
// gid below m, no position written twice, m rows in all.
int node_dict_export_parts(ngpu_node *node, const ngpu_dict *d, uint8_t *records) {
  ngpu_engine *e0 = node->eng[0];
  const uint64_t m = d->dev.m;
  const DictPlace *rows = d->place();
  uint64_t total = 0;
  for (const ngpu_dict *p : d->parts) total += p->dev.m;
  if (total != m)
    return fail(e0, NGPU_EINVAL, "node dict export: the parts do not tile the dict's ids (%llu rows, %llu entries)",
                (unsigned long long)total, (unsigned long long)m);
  if (!m) return 0;
  std::vector<uint64_t> seen((m + 63) / 64, 0);
  std::vector<DictRec> h(std::min<uint64_t>(m, 1u << 20));
  for (size_t o = 0; o < d->parts.size(); ++o) {
    const ngpu_dict *p = d->parts[o];
    const uint64_t m_o = p->dev.m;
    if (!m_o) continue;
    DeviceGuard dg(p->device);
    BuildStream bs(p->device);
    if (!bs.s) return fail(e0, NGPU_EHIP, "chunk dict: no build stream");
    for (uint64_t a = 0; a < m_o; a += h.size()) {
      const uint64_t c = std::min<uint64_t>(h.size(), m_o - a);
      if (hipMemcpyAsync(h.data(), p->st->rec + a, c * sizeof(DictRec), hipMemcpyDeviceToHost, bs.s) !=
              hipSuccess ||
          hipStreamSynchronize(bs.s) != hipSuccess)
        return fail(e0, NGPU_EHIP, "node dict export: copy of part %zu's records failed", o);
      for (uint64_t i = 0; i < c; ++i) {
        const uint64_t g = h[i].gid;
        if (g >= m || ((seen[g >> 6] >> (g & 63)) & 1))
          return fail(e0, NGPU_EINVAL,
                      "node dict export: the parts do not tile the dict's ids (id %llu of part %zu, %llu entries)",
                      (unsigned long long)g, o, (unsigned long long)m);
        seen[g >> 6] |= 1ull << (g & 63);
        dict_export_row(h[i], rows ? rows + g : nullptr, records + 80 * g);
      }
    }
  }
  return 0;
}

// ---- node dict fold ------------------------------------------------------------
// ngpu_dict_fold for node dicts: every part's result table becomes dict rows on
// its own device, and the rows reach the parts that keep them by DMA copies.
// Per part i, on engine i's fold stream and kept scratch (fold_mu, taken in index
// order):
//   a. dict fold's keep words, scan and layer ranks (launch_fold_keep_scan,
//      unchanged) and, for a partitioned base, its NEW chunks per owner
//      (fold_owner_counts); one 320-B copy into pinned memory brings back k_i,
//      b_i, the refusal counters and the W owner counts.  All W parts are
//      enqueued before the first wait, the call's only mid-way one.
//   b. the host plan (node_fold_plan.hpp): offsets, totals, segments, refusals --
//      all of them before any `used` is reserved or a storage byte is written.
//   c. launch_fold_scatter writes part i's rows into a staging area on device i
//      with their final global ids and blobs (sized for k = n before a., so the
//      keep words are never freed under the call).
//   d. partitioned: the stable split of the staged rows by owner (node_fold.hip).
//   e. each part's extend through dict_extend_rows: its write waits for the
//      source parts' "staged" events and copies a replica all W staging areas, a
//      partition its W segments, in source order (hipMemcpyAsync for its own,
//      hipMemcpyPeerAsync for the others); the insert or build follows unchanged.
//   f. the global handle's placement rows and blob table, as node_dict_extend.
struct NodeFoldRows {
  uint8_t *scr = nullptr;  // engine i's fold_scr
  FoldScratch lay;
  DictRec *staged = nullptr, *split = nullptr;
  uint32_t *tcnt = nullptr;
  uint64_t *tsums = nullptr;
};
constexpr uint64_t kNodeFoldCtrBytes = 8 * kFoldCtrWords + 4 * kNodeFoldMaxParts;  // counters + owner counts

// Part o's new rows into dst on s, in source order.  c: W x W owner counts (a
// partition takes its W segments), null: a replica takes all W staging areas.
void node_fold_write(ngpu_node *node, const NodeFoldPlan &plan, const std::vector<NodeFoldRows> &rows,
                     const uint32_t *c, uint32_t o, DictRec *dst, hipStream_t s) {
  const uint32_t W = (uint32_t)node->eng.size();
  for (uint32_t i = 0; i < W; ++i) {
    const uint64_t cnt = c ? c[(size_t)i * W + o] : plan.off[i + 1] - plan.off[i];
    if (!cnt) continue;
    const NodeFoldRows &r = rows[i];
    const DictRec *from = c ? r.split + plan.src[(size_t)i * W + o] : r.staged;
    DictRec *to = dst + (c ? plan.dst[(size_t)i * W + o] : plan.off[i]);
    if (i == o) {  // staged on this very stream
      (void)hipMemcpyAsync(to, from, cnt * sizeof(DictRec), hipMemcpyDeviceToDevice, s);
    } else if (hipStreamWaitEvent(s, node->eng[i]->fold_ev, 0) == hipSuccess) {
      (void)hipMemcpyPeerAsync(to, node->dev[o], from, node->dev[i], cnt * sizeof(DictRec), s);
    }
  }
}

// e->fold_mu held: at least `bytes` of fold_rows, the pinned counters and the event.
int node_fold_lane(ngpu_engine *e, uint64_t bytes) {
  if (!e->fold_h && hipHostMalloc((void **)&e->fold_h, 512) != hipSuccess) {
    (void)hipGetLastError();
    e->fold_h = nullptr;
    return fail(e, NGPU_ENOMEM, "node dict fold: pinned counters");
  }
  if (!e->fold_ev && hipEventCreateWithFlags(&e->fold_ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    e->fold_ev = nullptr;
    return fail(e, NGPU_EHIP, "node dict fold: event on device %d", e->device);
  }
  return grow_kept(e, &e->fold_rows, &e->fold_rows_cap, bytes,
                   "node dict fold: staging allocation failed");
}

int node_dict_fold(ngpu_node *node, ngpu_dict *base, const ngpu_node_fold_part *pt, uint32_t np,
                   const ngpu_dict_place *placements, uint64_t n_placements, const uint8_t *blobs,
                   uint32_t n_blobs, ngpu_dict **out) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (np != W)
    return fail(e0, NGPU_EINVAL, "node dict fold: %u parts for a node of %u devices", np, W);
  if (int rc = node_dict_base_check(node, base, "fold")) return rc;
  std::vector<uint64_t> L(W);
  std::vector<const uint64_t *> lfirst(W);
  for (uint32_t i = 0; i < W; ++i) {
    const ngpu_node_fold_part &p = pt[i];
    if ((p.n && (!p.d_results || !p.d_chunks)) || ((uintptr_t)p.d_results & 15) ||
        ((uintptr_t)p.d_chunks & 7) || ((uintptr_t)p.d_layer_first & 7))
      return fail(e0, NGPU_EINVAL, "node dict fold: part %u: missing or misaligned tables", i);
    if (p.n >= kDictMaxEntries || p.n_layers >= kDictMaxEntries)
      return fail(e0, NGPU_EINVAL, "node dict fold: part %u: %llu chunks in %llu layers in one call", i,
                  (unsigned long long)p.n, (unsigned long long)p.n_layers);
    const bool one = !p.d_layer_first || p.n_layers <= 1;  // one layer of n chunks
    lfirst[i] = one ? nullptr : p.d_layer_first;
    L[i] = one ? 1 : p.n_layers;
  }
  const bool split = !base->replicated;
  const uint64_t m = base->dev.m;
  std::vector<std::unique_lock<std::mutex>> lanes;
  for (uint32_t i = 0; i < W; ++i) lanes.emplace_back(node->eng[i]->fold_mu);

  // a. counts: every part enqueued, then waited for
  std::vector<NodeFoldRows> rows(W);
  int rc = 0;
  for (uint32_t i = 0; i < W && !rc; ++i) {
    ngpu_engine *e = node->eng[i];
    const ngpu_node_fold_part &p = pt[i];
    NodeFoldRows &r = rows[i];
    DeviceGuard dg(e->device);
    const uint64_t n = p.n;
    r.lay = fold_scratch_layout(n, L[i], kNodeFoldCtrBytes);
    // the staging areas for the worst case k = n, before the keep words exist
    const uint64_t tw = (uint64_t)W * node_split_tiles(n);
    const uint64_t o_split = n * sizeof(DictRec), o_tcnt = 2 * o_split,
                   o_tsums = (o_tcnt + 4 * tw + 7) & ~7ull,
                   bytes = split ? o_tsums + 8 * ((tw + kRetireScanTile - 1) / kRetireScanTile + 1) : o_split;
    if ((rc = fold_lane(e, r.lay.bytes)) || (rc = node_fold_lane(e, bytes))) {
      rc = fail(e0, rc, "%s", ngpu_last_error(e));
      break;
    }
    r.scr = e->fold_scr;
    r.staged = (DictRec *)e->fold_rows;
    if (split) {
      r.split = (DictRec *)(e->fold_rows + o_split);
      r.tcnt = (uint32_t *)(e->fold_rows + o_tcnt);
      r.tsums = (uint64_t *)(e->fold_rows + o_tsums);
    }
    const hipStream_t s = e->fold_stream;
    uint64_t *d_ctr = (uint64_t *)(r.scr + r.lay.ctr);
    bool ok = hipMemsetAsync(d_ctr, 0, kNodeFoldCtrBytes, s) == hipSuccess;
    if (ok) {
      launch_fold_keep_scan(p.d_results, p.d_chunks, n, e->cfg.chunk_size, lfirst[i], L[i],
                            (uint64_t *)(r.scr + r.lay.words), (uint32_t *)(r.scr + r.lay.cnt),
                            (uint64_t *)(r.scr + r.lay.sums), (uint32_t *)(r.scr + r.lay.rank), d_ctr, s);
      if (split) launch_fold_owner_counts(p.d_results, n, W, (uint32_t *)(d_ctr + kFoldCtrWords), s);
      ok = hipGetLastError() == hipSuccess &&
           hipMemcpyAsync(e->fold_h, d_ctr, kNodeFoldCtrBytes, hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    if (!ok) rc = fail(e0, NGPU_EHIP, "node dict fold: part %u: keep scan failed", i);
  }
  for (uint32_t i = 0; i < W; ++i) {  // (every stream is waited for, whatever another one said)
    DeviceGuard dg(node->dev[i]);
    const hipStream_t s = node->eng[i]->fold_stream;
    if (s && hipStreamSynchronize(s) != hipSuccess && !rc)
      rc = fail(e0, NGPU_EHIP, "node dict fold: part %u: keep scan failed", i);
  }
  if (rc) return rc;

  // b. the plan; every refusal comes before `used` is reserved or a storage byte is written
  std::vector<uint64_t> k(W), b(W);
  std::vector<uint32_t> c(split ? (size_t)W * W : 0);
  for (uint32_t i = 0; i < W; ++i) {
    const uint64_t *ctr = node->eng[i]->fold_h;
    const uint64_t n = pt[i].n;
    const FoldVerdict v = fold_counts_verdict(ctr, n, L[i]);
    char prefix[40];
    snprintf(prefix, sizeof prefix, "node dict fold: part %u: ", i);
    if (int r = fold_fail(e0, prefix, v, n, L[i])) return r;
    k[i] = v.k;
    b[i] = v.b;
    if (split) memcpy(&c[(size_t)i * W], ctr + kFoldCtrWords, 4 * W);
  }
  const NodeFoldPlan plan = node_fold_plan(W, k.data(), b.data(), split ? c.data() : nullptr);
  if (!plan.ok)
    return fail(e0, NGPU_EHIP, "node dict fold: part %u: its owner counts do not add up to its %llu NEW chunks",
                plan.bad, (unsigned long long)k[plan.bad]);
  const uint64_t K = plan.K;
  const bool call_table = blobs && n_blobs;
  const DictFoldPlace pr =
      node_fold_place_rule(m, base->has_place, placements != nullptr, n_placements, plan);
  if (int r = fold_place_fail(e0, "node dict fold: ", pr, n_placements, K,
                              node_fold_table_rows_ok(blobs != nullptr, n_blobs, plan), n_blobs, plan.B))
    return r;
  // (over the untruncated sums: dict_extend_check_blobs below takes a 32-bit blob count)
  const NodeFoldLimit lim = node_fold_limits(m, base->dev.n_blobs, K, plan.B);
  if (lim == kNodeFoldEntries)
    return fail(e0, NGPU_EINVAL, "chunk dict too large (%llu entries)", (unsigned long long)(m + K));
  if (lim == kNodeFoldBlobs)
    return fail(e0, NGPU_EINVAL, "chunk dict blob index %llu too large",
                (unsigned long long)(base->dev.n_blobs + plan.B - 1));
  uint32_t nb = 0;
  bool with_table = false;
  if (int r = dict_extend_check_blobs(e0, base, K, (uint32_t)plan.B, call_table, n_blobs, &nb, &with_table))
    return r;

  // c, d. the rows, staged with their final ids and blobs (and split by owner)
  for (uint32_t i = 0; i < W; ++i) {
    if (!k[i]) continue;
    ngpu_engine *e = node->eng[i];
    const ngpu_node_fold_part &p = pt[i];
    const NodeFoldRows &r = rows[i];
    DeviceGuard dg(e->device);
    const hipStream_t s = e->fold_stream;
    launch_fold_scatter(p.d_results, p.d_chunks, p.n, (const uint64_t *)(r.scr + r.lay.words),
                        (const uint32_t *)(r.scr + r.lay.cnt), lfirst[i], L[i],
                        (const uint32_t *)(r.scr + r.lay.rank), base->dev.n_blobs + (uint32_t)plan.boff[i],
                        (uint32_t)(m + plan.off[i]), r.staged, k[i], s);
    if (split) launch_node_split(r.staged, k[i], W, r.tcnt, r.tsums, r.split, s);
    if (hipGetLastError() != hipSuccess || hipEventRecord(e->fold_ev, s) != hipSuccess) {
      rc = fail(e0, NGPU_EHIP, "node dict fold: part %u: staging its rows failed", i);
      break;
    }
  }
  auto quiesce = [&] {  // nothing of this call still reads a scratch when it returns
    for (uint32_t i = 0; i < W; ++i) {
      DeviceGuard dg(node->dev[i]);
      (void)hipStreamSynchronize(node->eng[i]->fold_stream);
    }
  };
  if (rc) {
    quiesce();
    return rc;
  }

  // e, f. the handle: placement rows, every part's extend, the blob table
  ngpu_dict *d = dict_derive(base);
  d->dev.m = m + K;
  d->dev.n_blobs = nb;
  if (pr == kPlaceKept || K == 0)
    rc = dict_place_extend(e0, base, reinterpret_cast<const DictPlace *>(placements), K, d);
  for (uint32_t o = 0; o < W && !rc; ++o) {
    ngpu_dict *p = nullptr;
    const uint64_t pk = split ? plan.total[o] : K;
    auto write = [&](DictRec *dst, uint64_t, hipStream_t s) {
      node_fold_write(node, plan, rows, split ? c.data() : nullptr, o, dst, s);
    };
    DictRowSource src;
    if (pk) {
      src.write = std::ref(write);  // (a reference: no allocation for the captures)
      src.stream = node->eng[o]->fold_stream;
      src.name = "node_dict_fold";
      src.n = pt[o].n;
    }
    if ((rc = dict_extend_rows(node->eng[o], base->parts[o], src, pk, nb, false, &p))) {
      rc = fail(e0, rc, "%s", ngpu_last_error(node->eng[o]));
      break;
    }
    d->parts.push_back(p);
  }
  quiesce();
  if (rc) {
    dict_unref(d);
    return rc;
  }
  dict_merge_blob_table(d, base, with_table, blobs, n_blobs);
  *out = d;
  return 0;
}

}  // namespace

// Called by dict_unref for a node dict.
void node_dict_free(ngpu_dict *d) {
  for (auto &r : d->req) {
    for (size_t o = 0; o < r->io.size() && o < d->parts.size(); ++o) {
      ngpu_dict::PartIO &io = r->io[o];
      const int dev = d->parts[o]->device;
      free_io(io, dev);
      DeviceGuard g(dev);
      if (io.stream) (void)hipStreamDestroy(io.stream);
      if (io.done) (void)hipEventDestroy(io.done);
    }
    if (r->ready) {
      DeviceGuard g(r->device);
      (void)hipEventDestroy(r->ready);
    }
  }
  d->req.clear();
  for (ngpu_dict *p : d->parts) dict_unref(p);
  d->parts.clear();
}

// ---- node step ---------------------------------------------------------------
namespace {

// RCCL is loaded when a step first asks for it (dlopen): processes that never
// run an RCCL step do not map its 570 MB library or register its kernels.
struct Rccl {
  decltype(&ncclCommInitAll) init = nullptr;
  decltype(&ncclCommDestroy) destroy = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclAllToAllv) alltoallv = nullptr;
  decltype(&ncclGetErrorString) err = nullptr;
  bool ok = false;
};
const Rccl &rccl() {
  static const Rccl r = [] {
    Rccl x;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) return x;
    x.init = (decltype(x.init))dlsym(h, "ncclCommInitAll");
    x.destroy = (decltype(x.destroy))dlsym(h, "ncclCommDestroy");
    x.group_start = (decltype(x.group_start))dlsym(h, "ncclGroupStart");
    x.group_end = (decltype(x.group_end))dlsym(h, "ncclGroupEnd");
    x.alltoallv = (decltype(x.alltoallv))dlsym(h, "ncclAllToAllv");
    x.err = (decltype(x.err))dlsym(h, "ncclGetErrorString");
    x.ok = x.init && x.destroy && x.group_start && x.group_end && x.alltoallv && x.err;
    return x;
  }();
  return r;
}

void step_free(ngpu_node *node) {
  for (size_t i = 0; i < node->sb.size(); ++i) {
    StepBuf &b = node->sb[i];
    DeviceGuard g(node->dev[i]);
    if (b.done) (void)hipEventSynchronize(b.done);
    for (void *p : {(void *)b.xq, (void *)b.xrow, (void *)b.sh, (void *)b.hits, (void *)b.rq,
                    (void *)b.rh, (void *)b.cnt, (void *)b.rcnt})
      if (p) (void)hipFree(p);
    for (hipEvent_t ev : {b.counted, b.sent, b.returned, b.done})
      if (ev) (void)hipEventDestroy(ev);
  }
  node->sb.clear();
  for (ncclComm_t c : node->comms)
    if (c) (void)rccl().destroy(c);
  node->comms.clear();
}

// The node's RCCL communicator (one rank per device), created on first use.
int step_comms(ngpu_node *node) {
  ngpu_engine *e0 = node->eng[0];
  if (!node->comms.empty()) return 0;
  if (!rccl().ok) return fail(e0, NGPU_EUNSUPP, "node step over RCCL: librccl.so.1 not loadable");
  const int W = (int)node->dev.size();
  for (int a = 0; a < W; ++a)
    for (int b = a + 1; b < W; ++b)
      if (node->dev[a] == node->dev[b])
        return fail(e0, NGPU_EUNSUPP, "node step over RCCL: device %d is listed twice (RCCL "
                    "takes one rank per GPU)", node->dev[a]);
  std::vector<ncclComm_t> c((size_t)W);
  const ncclResult_t r = rccl().init(c.data(), W, node->dev.data());
  if (r != ncclSuccess)
    return fail(e0, NGPU_EHIP, "node step: ncclCommInitAll over %d devices: %s", W,
                rccl().err(r));
  node->comms = std::move(c);
  return 0;
}

// quiesce: waits for the previous step before a buffer it may still use is freed
template <class Q>
int step_grow(ngpu_engine *e, StepBuf &b, uint64_t n, uint64_t r, Q &&quiesce) {
  if (!b.cnt) HIP_TRY(e, hipMalloc((void **)&b.cnt, 128 * sizeof(uint32_t)));
  if (!b.rcnt) HIP_TRY(e, hipMalloc((void **)&b.rcnt, 64 * sizeof(uint32_t)));
  for (hipEvent_t *ev : {&b.counted, &b.sent, &b.returned, &b.done})
    if (!*ev) HIP_TRY(e, hipEventCreateWithFlags(ev, hipEventDisableTiming));
  if ((n > b.cap && b.xq) || (r > b.rcap && b.rq))
    if (int rc = quiesce()) return rc;
  if (n > b.cap || !b.xq) {
    for (void *p : {(void *)b.xq, (void *)b.xrow, (void *)b.sh, (void *)b.hits})
      if (p) (void)hipFree(p);
    b.xq = nullptr, b.xrow = nullptr, b.sh = nullptr, b.hits = nullptr, b.cap = 0;
    const uint64_t c = next_pow2(n < 1024 ? 1024 : n);
    HIP_TRY(e, hipMalloc((void **)&b.xq, c * 32));
    HIP_TRY(e, hipMalloc((void **)&b.xrow, c * 4));
    HIP_TRY(e, hipMalloc((void **)&b.sh, c * sizeof(ngpu_dict_hit)));
    HIP_TRY(e, hipMalloc((void **)&b.hits, c * sizeof(ngpu_dict_hit)));
    b.cap = c;
  }
  if (r > b.rcap || !b.rq) {
    if (b.rq) (void)hipFree(b.rq);
    if (b.rh) (void)hipFree(b.rh);
    b.rq = nullptr, b.rh = nullptr, b.rcap = 0;
    const uint64_t c = next_pow2(r < 1024 ? 1024 : r);
    HIP_TRY(e, hipMalloc((void **)&b.rq, c * 32));
    HIP_TRY(e, hipMalloc((void **)&b.rh, c * sizeof(ngpu_dict_hit)));
    b.rcap = c;
  }
  return 0;
}

#define NCCL_TRY(e, x)                                                                  \
  do {                                                                                  \
    const ncclResult_t r_ = (x);                                                        \
    if (r_ != ncclSuccess) return fail(e, NGPU_EHIP, "node step: %s: %s", #x, rccl().err(r_)); \
  } while (0)

// One all-to-all-v of `row`-byte rows: part i sends cnt_send(i, j) rows from
// src[i] + sdis(i, j) to part j, which stores them at dst[j] + rdis(j, i).
template <class CntF, class SdisF, class RdisF>
int step_alltoallv(ngpu_node *node, bool use_rccl, const std::vector<hipStream_t> &s,
                   const std::vector<const uint8_t *> &src, const std::vector<uint8_t *> &dst,
                   uint64_t row, CntF cnt_send, SdisF sdis, RdisF rdis, hipEvent_t StepBuf::*mark) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (use_rccl) {
    std::vector<size_t> sc(W), sd(W), rc(W), rd(W);
    NCCL_TRY(e0, rccl().group_start());
    for (uint32_t i = 0; i < W; ++i) {
      a2a_rank_args(W, i, row, cnt_send, sdis, rdis, sc.data(), sd.data(), rc.data(), rd.data());
      const ncclResult_t r = rccl().alltoallv(src[i], sc.data(), sd.data(), dst[i], rc.data(),
                                              rd.data(), ncclUint8, node->comms[i], s[i]);
      if (r != ncclSuccess) {
        (void)rccl().group_end();
        return fail(e0, NGPU_EHIP, "node step: ncclAllToAllv: %s", rccl().err(r));
      }
    }
    NCCL_TRY(e0, rccl().group_end());
    return 0;
  }
  // peer copies on the sender's stream; every receiver waits for every sender
  for (uint32_t i = 0; i < W; ++i) {
    DeviceGuard g(node->dev[i]);
    for (uint32_t j = 0; j < W; ++j) {
      const uint64_t c = cnt_send(i, j);
      if (c)
        HIP_TRY(e0, hipMemcpyPeerAsync(dst[j] + rdis(j, i) * row, node->dev[j],
                                       src[i] + sdis(i, j) * row, node->dev[i], c * row, s[i]));
    }
    HIP_TRY(e0, hipEventRecord(node->sb[i].*mark, s[i]));
  }
  for (uint32_t j = 0; j < W; ++j) {
    DeviceGuard g(node->dev[j]);
    for (uint32_t i = 0; i < W; ++i)
      if (i != j) HIP_TRY(e0, hipStreamWaitEvent(s[j], node->sb[i].*mark, 0));
  }
  return 0;
}

int node_step_enqueue(ngpu_node *node, ngpu_dict *d, const ngpu_node_part *pt, uint32_t W,
                      bool use_rccl);

// A failed step may have enqueued part of its work on the parts' streams: it
// is waited for before the step buffers can be reused (or freed).
int node_step(ngpu_node *node, ngpu_dict *d, const ngpu_node_part *pt, uint32_t np, uint32_t flags) {
  ngpu_engine *e0 = node->eng[0];
  const uint32_t W = (uint32_t)node->eng.size();
  if (np != W) return fail(e0, NGPU_EINVAL, "node step: %u parts for a node of %u devices", np, W);
  for (uint32_t i = 0; i < W; ++i) {
    const ngpu_node_part &p = pt[i];
    if ((p.n && (!p.d_data || !p.d_chunks || !p.d_out)) || (p.d_layer_first && !p.n_layers) ||
        p.n >= 0xFFFFFFFFull)
      return fail(e0, NGPU_EINVAL, "node step: bad part %u", i);
  }
  if (!d || d->parts.empty() || d->replicated) {  // no exchange: each part on its own
    for (uint32_t i = 0; i < W; ++i) {
      const ngpu_node_part &p = pt[i];
      if (int rc = ngpu_process_dict_device(node->eng[i], d, p.d_data, p.len, p.d_chunks, p.n,
                                            p.d_out, p.d_layer_first, p.n_layers, p.d_stats,
                                            p.stream, nullptr))
        return rc;
    }
    return 0;
  }
  if (d->parts.size() != W) return fail(e0, NGPU_EINVAL, "node step: the dict has %zu parts, the node %u devices",
                                        d->parts.size(), W);
  for (uint32_t i = 0; i < W; ++i)
    if (d->parts[i]->device != node->dev[i])
      return fail(e0, NGPU_EINVAL, "node step: dict part %u is not on node device %u", i, i);
  const bool use_rccl = (flags & NGPU_NODE_STEP_RCCL) != 0;
  std::lock_guard<std::mutex> g(node->step_mu);
  if (use_rccl)
    if (int rc = step_comms(node)) return rc;
  const int rc = node_step_enqueue(node, d, pt, W, use_rccl);
  if (rc) {
    for (uint32_t i = 0; i < W; ++i) {
      DeviceGuard dg(node->dev[i]);
      (void)hipStreamSynchronize((hipStream_t)pt[i].stream);
    }
    node->stepped = false;  // nothing of this step is still in flight
  }
  return rc;
}

int node_step_enqueue(ngpu_node *node, ngpu_dict *d, const ngpu_node_part *pt, uint32_t W,
                      bool use_rccl) {
  ngpu_engine *e0 = node->eng[0];
  node->sb.resize(W);
  bool quiet = !node->stepped;
  auto quiesce = [&]() -> int {  // the previous step done on every device
    for (uint32_t j = 0; j < W && !quiet; ++j) {
      DeviceGuard dg(node->dev[j]);
      HIP_TRY(e0, hipEventSynchronize(node->sb[j].done));
    }
    quiet = true;
    return 0;
  };
  std::vector<hipStream_t> s(W);
  for (uint32_t i = 0; i < W; ++i) s[i] = (hipStream_t)pt[i].stream;
  // the padded layout (a2a_plan.hpp): every transfer size is known here, the
  // per-owner counts travel in band, and nothing below waits for the device
  std::vector<uint64_t> n(W), off(W + 1, 0);
  for (uint32_t i = 0; i < W; ++i) n[i] = pt[i].n, off[i + 1] = off[i] + n[i];
  if (W > 64) return fail(e0, NGPU_EINVAL, "node step: %u parts (at most 64)", W);
  const PaddedStep ps{W, n.data(), off.data()};
  // buffers are reused: this step's streams start after every part of the last
  for (uint32_t i = 0; i < W; ++i) {
    DeviceGuard dg(node->dev[i]);
    if (int rc = step_grow(node->eng[i], node->sb[i], (uint64_t)W * n[i], off[W], quiesce))
      return rc;
    if (node->stepped)
      for (uint32_t j = 0; j < W; ++j) HIP_TRY(e0, hipStreamWaitEvent(s[i], node->sb[j].done, 0));
  }
  // 1. digests; 2. bucketed by owner into padded segments (seg_cap = n), the
  // padding rows' ids ~0
  for (uint32_t i = 0; i < W; ++i) {
    const ngpu_node_part &p = pt[i];
    StepBuf &b = node->sb[i];
    if (p.n)
      if (int rc = ngpu_digest_device(node->eng[i], p.d_data, p.len, p.d_chunks, p.n, p.d_out, p.stream))
        return rc;
    DeviceGuard dg(node->dev[i]);
    if (p.n) HIP_TRY(e0, hipMemsetAsync(b.xrow, 0xFF, (size_t)W * p.n * sizeof(uint32_t), s[i]));
    launch_route(reinterpret_cast<const uint8_t *>(p.d_out), sizeof(ngpu_result), p.n, W, p.n,
                 b.cnt, b.xq, b.xrow, s[i]);
    HIP_TRY(e0, hipGetLastError());
  }
  std::vector<const uint8_t *> src(W);
  std::vector<uint8_t *> dst(W);
  // 3. counts (requester i's cnt[j] -> owner j's rcnt[i]) and digests to their owners
  for (uint32_t i = 0; i < W; ++i)
    src[i] = reinterpret_cast<const uint8_t *>(node->sb[i].cnt),
    dst[i] = reinterpret_cast<uint8_t *>(node->sb[i].rcnt);
  if (int rc = step_alltoallv(node, use_rccl, s, src, dst, sizeof(uint32_t), PaddedStep::cnt_cnt,
                              PaddedStep::cnt_sdis, PaddedStep::cnt_rdis, &StepBuf::counted))
    return rc;
  for (uint32_t i = 0; i < W; ++i) src[i] = node->sb[i].xq, dst[i] = node->sb[i].rq;
  if (int rc = step_alltoallv(
          node, use_rccl, s, src, dst, 32, [&](uint32_t i, uint32_t j) { return ps.fwd_cnt(i, j); },
          [&](uint32_t i, uint32_t j) { return ps.fwd_sdis(i, j); },
          [&](uint32_t j, uint32_t i) { return ps.fwd_rdis(j, i); }, &StepBuf::sent))
    return rc;
  // 4. owners probe the counted rows of each requester's block
  ProbeBlocks pb{};
  pb.W = W;
  for (uint32_t i = 0; i <= W; ++i) pb.off[i] = off[i];
  for (uint32_t j = 0; j < W; ++j) {
    DeviceGuard dg(node->dev[j]);
    launch_dict_probe_blocks(node->sb[j].rq, node->sb[j].rcnt, pb, d->parts[j]->dev, node->sb[j].rh,
                             s[j]);
    HIP_TRY(e0, hipGetLastError());
  }
  // 5. hits back: owner j sends requester i's block to i's segment j
  for (uint32_t j = 0; j < W; ++j)
    src[j] = reinterpret_cast<const uint8_t *>(node->sb[j].rh),
    dst[j] = reinterpret_cast<uint8_t *>(node->sb[j].sh);
  if (int rc = step_alltoallv(
          node, use_rccl, s, src, dst, sizeof(ngpu_dict_hit),
          [&](uint32_t j, uint32_t i) { return ps.back_cnt(j, i); },
          [&](uint32_t j, uint32_t i) { return ps.back_sdis(j, i); },
          [&](uint32_t i, uint32_t j) { return ps.back_rdis(i, j); }, &StepBuf::returned))
    return rc;
  // 6. hits to their rows (padding rows dropped by their ~0 id), then each
  // part's own dedup
  const uint32_t nb = d->dev.n_blobs ? d->dev.n_blobs : 1;
  for (uint32_t i = 0; i < W; ++i) {
    const ngpu_node_part &p = pt[i];
    StepBuf &b = node->sb[i];
    ngpu_engine *e = node->eng[i];
    if (p.n) {
      DeviceGuard dg(e->device);
      launch_hits_scatter(b.sh, b.xrow, (uint64_t)W * p.n, b.hits, s[i]);
      HIP_TRY(e0, hipGetLastError());
      std::lock_guard<std::mutex> eg(e->mu);
      if (int rc = enqueue_dedup(e, nullptr, p.d_chunks, p.n, p.d_out, b.hits, nb, s[i],
                                 p.d_layer_first, p.d_layer_first ? p.n_layers : 1, p.d_stats))
        return rc;
    }
    DeviceGuard dg(node->dev[i]);
    HIP_TRY(e0, hipEventRecord(b.done, s[i]));
  }
  node->stepped = true;
  return 0;
}

}  // namespace

}  // namespace ngpu

extern "C" {

int ngpu_node_create(const int32_t *devices, uint32_t n, const ngpu_config *cfg, ngpu_node **out) {
  if (!devices || !n || n > 64 || !out) return NGPU_EINVAL;
  *out = nullptr;
  ngpu_node *node = new ngpu_node();
  for (uint32_t i = 0; i < n; ++i) {
    ngpu_config c{};
    if (cfg) c = *cfg;
    c.device = devices[i];
    ngpu_engine *e = nullptr;
    const int rc = ngpu_create(&c, &e);
    if (rc) {
      ngpu_node_destroy(node);
      return rc;
    }
    node->eng.push_back(e);
    node->dev.push_back(devices[i]);
  }
  // xGMI peer access between every pair of distinct devices (the exchange
  // copies go device to device)
  for (uint32_t a = 0; a < n; ++a)
    for (uint32_t b = 0; b < n; ++b) {
      if (node->dev[a] == node->dev[b]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, node->dev[a], node->dev[b]) != hipSuccess || !can) {
        (void)hipGetLastError();
        node->peer_ok = false;  // partitioned dicts fall back to the copy exchange
        continue;
      }
      DeviceGuard g(node->dev[a]);
      const hipError_t st = hipDeviceEnablePeerAccess(node->dev[b], 0);
      if (st != hipSuccess && st != hipErrorPeerAccessAlreadyEnabled) {
        ngpu_node_destroy(node);
        return NGPU_EHIP;
      }
      (void)hipGetLastError();
    }
  *out = node;
  return 0;
}

void ngpu_node_destroy(ngpu_node *node) {
  if (!node) return;
  {
    std::vector<ngpu_dict *> cache;
    {
      std::lock_guard<std::mutex> g(node->cache_mu);
      cache.swap(node->dict_cache);
    }
    for (ngpu_dict *d : cache) dict_unref(d);  // the cache's references (packs keep their own)
  }
  step_free(node);
  for (ngpu_engine *e : node->eng) ngpu_destroy(e);
  delete node;
}

uint32_t ngpu_node_size(const ngpu_node *node) { return node ? (uint32_t)node->eng.size() : 0; }

ngpu_engine *ngpu_node_engine(ngpu_node *node, uint32_t i) {
  return node && i < node->eng.size() ? node->eng[i] : nullptr;
}

uint32_t ngpu_node_owner(const ngpu_node *node, const uint8_t *digest) {
  return node && digest ? owner_of(digest, (uint32_t)node->eng.size()) : 0;
}

int ngpu_node_dict_create(ngpu_node *node, const void *records, uint64_t n,
                          const void *blob_table, uint32_t n_blobs, uint32_t mode,
                          ngpu_dict **out) {
  if (!node || !out || (n && !records) || (n_blobs && !blob_table)) return NGPU_EINVAL;
  *out = nullptr;
  return guarded([&] {
    return node_dict_build(node, (const uint8_t *)records, n, (const uint8_t *)blob_table, n_blobs,
                           mode, out);
  });
}

int ngpu_node_dict_extend(ngpu_node *node, ngpu_dict *base, const void *records, uint64_t n,
                          const void *blob_table, uint32_t n_blobs, uint32_t flags,
                          ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !node || !out || (n && !records) || (n_blobs && !blob_table))
    return NGPU_EINVAL;
  return guarded([&] {
    return node_dict_extend(node, base, (const uint8_t *)records, n, (const uint8_t *)blob_table,
                            n_blobs, out);
  });
}

int ngpu_node_dict_retire(ngpu_node *node, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                          uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !node || !out || (n && !blobs)) return NGPU_EINVAL;
  return guarded([&] { return node_dict_retire(node, base, blobs, n, out); });
}

int ngpu_node_dict_retire_parts(ngpu_node *node, ngpu_dict *base, const uint32_t *blobs, uint32_t n,
                                uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !node || !out || (n && !blobs)) return NGPU_EINVAL;
  return guarded([&] { return node_dict_retire_parts(node, base, blobs, n, out); });
}

int ngpu_node_dict_distill(ngpu_node *node, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                           ngpu_dict **out, ngpu_dict_distill_info *info) {
  if (out) *out = nullptr;
  if (info) memset(info, 0, sizeof *info);
  if (!base || !node || dict_distill_args(flags)) return NGPU_EINVAL;
  return guarded([&]() -> int {
    ngpu_dict_distill_info got;
    memset(&got, 0, sizeof got);
    const int rc = node_dict_distill(node, base, min_refs, flags, out, &got);
    if (!rc && info) *info = got;
    return rc;
  });
}

int ngpu_node_dict_distill_parts(ngpu_node *node, ngpu_dict *base, uint32_t min_refs, uint32_t flags,
                                 ngpu_dict **out, ngpu_dict_distill_info *info) {
  if (out) *out = nullptr;
  if (info) memset(info, 0, sizeof *info);
  if (!base || !node || dict_distill_args(flags)) return NGPU_EINVAL;
  return guarded([&]() -> int {
    ngpu_dict_distill_info got;
    memset(&got, 0, sizeof got);
    const int rc = node_dict_distill_parts(node, base, min_refs, flags, out, &got);
    if (!rc && info) *info = got;
    return rc;
  });
}

static_assert(sizeof(ngpu_node_dict_remode_options) == 16, "ngpu_node_dict_remode_options is 16 bytes");
static_assert(sizeof(ngpu_node_dict_info) == 528, "ngpu_node_dict_info is 528 bytes");

int ngpu_node_dict_remode(ngpu_node *node, ngpu_dict *base, uint32_t mode,
                          const ngpu_node_dict_remode_options *opt, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!node || !base || !out || (opt && (opt->flags || opt->reserved))) return NGPU_EINVAL;
  const uint64_t window_records = opt ? opt->window_records : 0;
  const int rc = guarded([&] { return node_dict_remode(node, base, mode, window_records, out); });
  if (rc) *out = nullptr;
  return rc;
}

int ngpu_node_dict_info_get(const ngpu_node *node, const ngpu_dict *d, ngpu_node_dict_info *out) {
  if (out) memset(out, 0, sizeof *out);
  if (!node || !d || !out) return NGPU_EINVAL;
  if (d->parts.empty())
    return fail(node->eng[0], NGPU_EINVAL, "node dict info: not a node dict (ngpu_dict_info_get takes it)");
  if (int rc = node_dict_base_check(const_cast<ngpu_node *>(node), d, "info")) return rc;
  out->mode = d->replicated ? NGPU_NODE_DICT_REPLICATE
                            : NGPU_NODE_DICT_PARTITION |
                                  (d->routed ? NGPU_NODE_EXCHANGE_ROUTED : NGPU_NODE_EXCHANGE_COPY);
  out->parts = (uint32_t)d->parts.size();
  out->entries = d->dev.m;
  for (size_t i = 0; i < d->parts.size() && i < 64; ++i) out->part_entries[i] = d->parts[i]->dev.m;
  return 0;
}

int ngpu_node_dict_export(ngpu_node *node, const ngpu_dict *d, void *records, uint64_t cap,
                          uint64_t *n_records, void *blob_table, uint32_t blob_cap, uint32_t *n_blobs,
                          uint32_t flags) {
  if (n_records) *n_records = d ? d->dev.m : 0;
  if (n_blobs) *n_blobs = d ? d->dev.n_blobs : 0;
  if (!node || !d || !n_records || !n_blobs || flags) return NGPU_EINVAL;
  return guarded([&]() -> int {
    ngpu_engine *e0 = node->eng[0];
    if (int rc = node_dict_base_check(node, d, "export")) return rc;
    if (d->replicated)
      return ngpu_dict_export(e0, d, records, cap, n_records, blob_table, blob_cap, n_blobs);
    const uint64_t m = d->dev.m;
    if (!records && !cap) return 0;  // a count
    if (cap < m || (m && !records))
      return fail(e0, NGPU_EINVAL, "node dict export: room for %llu of %llu records",
                  (unsigned long long)cap, (unsigned long long)m);
    const bool table = blob_table && !d->blob_table.empty();
    if (table && 256ull * blob_cap < d->blob_table.size())
      return fail(e0, NGPU_EINVAL, "node dict export: room for %u of %llu blob records", blob_cap,
                  (unsigned long long)(d->blob_table.size() / 256));
    if (int rc = node_dict_export_parts(node, d, (uint8_t *)records)) return rc;
    if (table) memcpy(blob_table, d->blob_table.data(), d->blob_table.size());
    return 0;
  });
}

int ngpu_node_dict_save(ngpu_node *node, const ngpu_dict *d, const ngpu_dict_save_options *opt,
                        ngpu_write_fn w, void *ctx, ngpu_dict_save_info *info) {
  if (info) memset(info, 0, sizeof *info);
  if (!node || !d || !w) return NGPU_EINVAL;
  const int rc = guarded([&]() -> int {
    if (int rc = node_dict_base_check(node, d, "save")) return rc;
    return dict_save_run(node->eng[0], d, opt, true, w, ctx, info);
  });
  if (rc == NGPU_ENOMEM) fail(node->eng[0], rc, "node dict save: out of memory");
  return rc;
}

static_assert(sizeof(ngpu_node_fold_part) == 40, "ngpu_node_fold_part is 40 bytes");

int ngpu_node_dict_fold(ngpu_node *node, ngpu_dict *base, const ngpu_node_fold_part *parts,
                        uint32_t n_parts, const ngpu_dict_place *placements, uint64_t n_placements,
                        const void *blob_table, uint32_t n_blobs, uint32_t flags, ngpu_dict **out) {
  if (out) *out = nullptr;
  if (!base || flags || !node || !out || !parts || (n_placements && !placements) ||
      (n_blobs && !blob_table))
    return NGPU_EINVAL;
  return guarded([&] {
    return node_dict_fold(node, base, parts, n_parts, placements, n_placements,
                          (const uint8_t *)blob_table, n_blobs, out);
  });
}

int ngpu_node_dict_open(ngpu_node *node, const char *path, uint32_t mode, ngpu_dict **out) {
  if (!node || !path || !out) return NGPU_EINVAL;
  *out = nullptr;
  return guarded([&] {
    struct stat st;
    ngpu_engine *e0 = node->eng[0];
    if (stat(path, &st) != 0) return fail(e0, NGPU_EIO, "stat chunk dict %s", path);
    const int64_t mt = (int64_t)st.st_mtim.tv_sec * 1000000000 + st.st_mtim.tv_nsec;
    auto same = [&](const ngpu_dict *d) {
      return d->path == path && d->node_mode == mode && d->st_dev == (uint64_t)st.st_dev &&
             d->st_ino == (uint64_t)st.st_ino && d->st_size == (uint64_t)st.st_size &&
             d->st_mtime_ns == mt;
    };
    std::vector<ngpu_dict *> drop;
    {
      std::lock_guard<std::mutex> g(node->cache_mu);
      for (ngpu_dict *d : node->dict_cache)
        if (same(d)) {
          dict_ref(d);
          *out = d;
          return 0;
        }
    }
    std::vector<uint8_t> recs, blobs;
    if (int rc = read_dict_bootstrap(e0, path, (uint64_t)st.st_size, &recs, &blobs)) return rc;
    ngpu_dict *d = nullptr;
    if (int rc = node_dict_build(node, recs.data(), recs.size() / 80, blobs.data(),
                                 (uint32_t)(blobs.size() / 256), mode, &d))
      return rc;
    d->path = path;
    d->node_mode = mode;
    d->st_dev = (uint64_t)st.st_dev;
    d->st_ino = (uint64_t)st.st_ino;
    d->st_size = (uint64_t)st.st_size;
    d->st_mtime_ns = mt;
    {
      std::lock_guard<std::mutex> g(node->cache_mu);
      auto &c = node->dict_cache;
      for (ngpu_dict *x : c)
        if (same(x)) {  // another thread loaded it meanwhile: share that one
          dict_ref(x);
          drop.push_back(d);
          d = x;
          break;
        }
      if (std::find(c.begin(), c.end(), d) == c.end()) {
        for (size_t i = 0; i < c.size();)  // older loads of the path (same mode) go
          if (c[i]->path == path && c[i]->node_mode == mode) {
            drop.push_back(c[i]);
            c.erase(c.begin() + (long)i);
          } else {
            ++i;
          }
        if (c.size() >= 8) {
          drop.push_back(c.front());
          c.erase(c.begin());
        }
        dict_ref(d);  // the cache's reference
        c.push_back(d);
      }
    }
    for (ngpu_dict *x : drop) dict_unref(x);
    *out = d;
    return 0;
  });
}

// Layers shard over the node's GPUs (north star; convert_unix.go:467-538 runs
// one per goroutine): each Pack goes to the engine with the fewest open packs,
// the search starting one further each time so that ties rotate.
int ngpu_node_pack_open(ngpu_node *node, ngpu_dict *dict, uint32_t flags, ngpu_pack **out) {
  if (!node || !out) return NGPU_EINVAL;
  const size_t W = node->eng.size();
  std::lock_guard<std::mutex> g(node->place_mu);
  const uint64_t r = node->rr.fetch_add(1, std::memory_order_relaxed);
  size_t best = r % W;
  int load = node->eng[best]->open_packs.load();
  for (size_t k = 1; k < W; ++k) {
    const size_t i = (r + k) % W;
    const int l = node->eng[i]->open_packs.load();
    if (l < load) best = i, load = l;
  }
  return ngpu_pack_open_dict(node->eng[best], dict, flags, out);
}

int ngpu_node_process_device(ngpu_node *node, uint32_t i, ngpu_dict *dict, const void *d_data,
                             uint64_t len, const ngpu_chunk *d_chunks, uint64_t n,
                             ngpu_result *d_out, const uint64_t *d_layer_first,
                             uint64_t n_layers, ngpu_layer_stats *d_stats, void *stream) {
  if (!node || i >= node->eng.size()) return NGPU_EINVAL;
  return ngpu_process_dict_device(node->eng[i], dict, d_data, len, d_chunks, n, d_out,
                                  d_layer_first, n_layers, d_stats, stream, nullptr);
}

int ngpu_node_process_step(ngpu_node *node, ngpu_dict *dict, const ngpu_node_part *parts,
                           uint32_t n_parts, uint32_t flags) {
  if (!node || !parts || (flags & ~NGPU_NODE_STEP_RCCL)) return NGPU_EINVAL;
  return guarded([&] { return node_step(node, dict, parts, n_parts, flags); });
}

}  // extern "C"
