#!/usr/bin/env python3
"""Verity (ngpu_verity_device / ngpu_verity_image) measurements for DESIGN §3.

  python tools/verity_bench.py --device   # the tree of an image resident in HBM
  python tools/verity_bench.py --host     # Engine.verity of 2 GiB in host memory

--device: a 4 GiB random image in HBM; `calls` back-to-back ngpu_verity_device
  calls between two HIP events, alternated for `rounds` rounds with the only
  way the engine had to the same leaf digests before: ngpu_digest_device on a
  sha256 engine over the same bytes described as 512-byte chunk descriptors.
  Then whole trees of small images (one dependent chain per launch: the
  latency floor of a level) and one 16 GiB image.  The time of the levels
  above the leaves of the 4 GiB tree is read from a kernel trace of this
  command (verity_level against verity_leaves).  Reports GB/s of
  image bytes and the share of the 39.3 T op/s integer peak at 1,384 ops per
  compression, counting every compression of the tree.
--host: Engine.verity on 2 GiB in host memory (the call ends synchronised),
  against a 16-thread hashlib build of the same tree timed in the same run.
One JSON object per measurement on stdout."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch  # before the library: one HIP runtime per process
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nydus-snapshotter_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import nydus_gpu  # noqa: E402

GiB = 1 << 30
OPS_PER_COMPRESSION = 1384
PEAK_OPS = 39.3e12           # integer VALU peak the project measures against


def level_blocks(data_blocks):
    out, n = [], data_blocks
    while n > 1 or not out:
        if data_blocks == 1:
            return []
        n = -(-n // 128)
        out.append(n)
    return out


def compressions(data_blocks):
    """64-byte compressions of the whole tree: 9 per data block (8 + padding),
    65 per hash block (the top one's digest is the root)."""
    return 9 * data_blocks + 65 * sum(level_blocks(data_blocks))


def random_device(nbytes, seed):
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    for s in range(0, nbytes, GiB):
        buf[s:min(nbytes, s + GiB)].random_(0, 256, generator=g)
    return buf


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def rates(nbytes, ms):
    blocks = nbytes // 512
    return {"ms": round(ms, 4), "GBps_image": round(nbytes / ms / 1e6, 1),
            "peak_fraction": round(compressions(blocks) * OPS_PER_COMPRESSION / (ms * 1e-3) / PEAK_OPS, 3)}


def device_stage(calls, rounds, big):
    nbytes = 4 * GiB
    blocks = nbytes // 512
    buf = random_device(nbytes, 7)
    lay = nydus_gpu.verity_layout(nbytes)
    d_tree = torch.full((lay["tree_bytes"],), 0xFF, dtype=torch.uint8, device="cuda")
    d_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
    ch = np.zeros(blocks, nydus_gpu.CHUNK_DTYPE)
    ch["offset"] = np.arange(blocks, dtype=np.uint64) * np.uint64(512)
    ch["length"] = 512
    d_ch = torch.from_numpy(ch.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(blocks * 64, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    out = []
    with nydus_gpu.Engine(digester="sha256", chunk_size=0x1000) as eng:
        def verity():
            eng.verity_device(buf.data_ptr(), nbytes, d_tree.data_ptr(), d_root.data_ptr(), stream=s)

        def digest():
            eng.digest_device(buf.data_ptr(), nbytes, d_ch.data_ptr(), blocks, d_out.data_ptr(), stream=s)
        verity()
        digest()
        torch.cuda.synchronize()
        # the two agree on the leaves: level 0 is the chunk digests, in order
        first0 = sum(level_blocks(blocks)[1:]) * 4096
        lvl0 = d_tree[first0:first0 + 32 * blocks].view(blocks, 32)
        assert torch.equal(lvl0, d_out.view(blocks, 64)[:, :32]), "level 0 differs from the chunk digests"
        # spot check of the first hash block and the root's chain on the host
        hb = d_tree[first0:first0 + 4096].cpu().numpy().tobytes()
        assert hb[:32] == hashlib.sha256(buf[:512].cpu().numpy().tobytes()).digest()
        assert d_root.cpu().numpy().tobytes() == hashlib.sha256(d_tree[:4096].cpu().numpy().tobytes()).digest()
        t = {"verity": [], "digest": []}
        for _ in range(rounds):
            for name, fn in (("verity", verity), ("digest", digest)):
                t[name].append(timed(fn, calls))
        mv, md = statistics.median(t["verity"]), statistics.median(t["digest"])
        out.append({"measure": "device_4GiB", "image_bytes": nbytes, "data_blocks": blocks,
                    "tree_bytes": lay["tree_bytes"], "levels": lay["levels"], "calls_per_window": calls,
                    "verity_ms": [round(x, 4) for x in t["verity"]],
                    "digest512_ms": [round(x, 4) for x in t["digest"]],
                    "verity": rates(nbytes, mv),
                    "digest512": {"ms": round(md, 4), "GBps_image": round(nbytes / md / 1e6, 1),
                                  "peak_fraction": round(9 * blocks * OPS_PER_COMPRESSION / (md * 1e-3) / PEAK_OPS, 3)},
                    "verity_vs_digest512": round(md / mv, 3)})
        out.append(small_trees(eng, d_tree, calls, rounds, s))
        eng.device_status()
        del d_ch, d_out, lvl0
        if big:
            del buf, d_tree
            torch.cuda.empty_cache()
            nbytes = 16 * GiB
            buf = random_device(nbytes, 9)
            lay = nydus_gpu.verity_layout(nbytes)
            d_tree = torch.full((lay["tree_bytes"],), 0xFF, dtype=torch.uint8, device="cuda")
            verity()
            torch.cuda.synchronize()
            ts = [timed(verity, max(2, calls // 4)) for _ in range(rounds)]
            out.append({"measure": "device_16GiB", "image_bytes": nbytes, "tree_bytes": lay["tree_bytes"],
                        "levels": lay["levels"], "verity_ms": [round(x, 4) for x in ts],
                        "verity": rates(nbytes, statistics.median(ts))})
            eng.device_status()
    return out


def small_trees(eng, d_tree, calls, rounds, s):
    """Whole trees of small images (the first bytes of the big tree serve as
    data): with so few lanes every launch is one dependent chain, so these
    times are the latency floor of a level -- 9 compressions for the leaves,
    65 for each launch above them.  The split of the 4 GiB tree's own time
    between verity_leaves and verity_level comes from a kernel trace
    (rocprofv3 --kernel-trace --stats) of this same command, in a run of its own."""
    res = {"measure": "small_trees"}
    for blocks in (1, 128, 129, 16385):
        nbytes = blocks * 512
        lay = nydus_gpu.verity_layout(nbytes)
        img = d_tree[:nbytes]
        t_small = torch.empty(max(lay["tree_bytes"], 16), dtype=torch.uint8, device="cuda")
        r = torch.zeros(32, dtype=torch.uint8, device="cuda")

        def small():
            eng.verity_device(img.data_ptr(), nbytes, t_small.data_ptr(), r.data_ptr(), stream=s)
        small()
        torch.cuda.synchronize()
        ts = [timed(small, calls * 5) for _ in range(rounds)]
        res[f"{blocks}_blocks"] = {"launches": lay["levels"] + 1, "ms": round(statistics.median(ts), 4)}
    return res


def host_tree(data, threads):
    """The same tree with hashlib on `threads` threads (hashlib releases the GIL)."""
    def digests(buf, size):
        n = len(buf) // size
        parts = np.array_split(np.arange(n), threads * 4)

        def work(ix):
            return b"".join(hashlib.sha256(buf[i * size:(i + 1) * size]).digest() for i in ix)
        with ThreadPoolExecutor(threads) as ex:
            return b"".join(ex.map(work, parts))
    cur, levels = digests(memoryview(data), 512), []
    while True:
        pad = -len(cur) % 4096
        blk = cur + bytes(pad)
        levels.append(blk)
        cur = digests(memoryview(blk), 4096)
        if len(blk) == 4096:
            break
    return b"".join(reversed(levels)), cur


def host_pipeline(reps):
    nbytes = 2 * GiB
    data = np.random.default_rng(11).integers(0, 256, nbytes, dtype=np.uint8)
    out = []
    t_cpu = []
    for _ in range(max(1, reps - 1)):
        t0 = time.perf_counter()
        ref_tree, ref_root = host_tree(data, 16)
        t_cpu.append(time.perf_counter() - t0)
    out.append({"measure": "cpu_tree_hashlib_16_threads", "bytes": nbytes, "s": [round(x, 3) for x in t_cpu],
                "GBps": round(nbytes / min(t_cpu) / 1e9, 2)})
    with nydus_gpu.Engine() as eng:
        tree, info = eng.verity(data)  # warm-up: pins the two windows (kept in the engine's pool)
        assert tree.tobytes() == ref_tree and info["root"] == ref_root.hex()
        for want_tree in (True, False):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng.verity(data, want_tree=want_tree)
                ts.append(time.perf_counter() - t0)
            out.append({"measure": "host_pipeline", "bytes": nbytes, "tree_returned": want_tree,
                        "s": [round(x, 4) for x in ts], "GBps_image": round(nbytes / min(ts) / 1e9, 2),
                        "vs_cpu_16_threads": round(min(t_cpu) / min(ts), 2),
                        "share_of_54GBps_h2d": round(nbytes / min(ts) / 54e9, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-16g", action="store_true", help="--device: skip the 16 GiB image")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("verity_bench: no GPU (there is no CPU fallback)")
    if args.device or not args.host:
        for r in device_stage(args.calls, args.rounds, not args.no_16g):
            print(json.dumps(r), flush=True)
    if args.host or not args.device:
        for r in host_pipeline(args.reps):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
