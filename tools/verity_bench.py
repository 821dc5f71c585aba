#!/usr/bin/env python3
"""Verity (ngpu_verity_device / ngpu_verity_image) measurements for DESIGN §3.

  python tools/verity_bench.py --device   # the tree of an image resident in HBM
  python tools/verity_bench.py --host     # Engine.verity of 2 GiB in host memory
  python tools/verity_bench.py --verify-device   # verify against the build, images in HBM
  python tools/verity_bench.py --verify-host     # Engine.verity_verify against rebuild-and-compare

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
--verify-device: verify (ngpu_verity_verify_tree_device + _data_device) of 4 GiB
  and 16 GiB images and their stored trees in HBM between two HIP events,
  alternated round by round with ngpu_verity_device on the same bytes.
--verify-host: Engine.verity_verify of 2 GiB in host memory, alternated with
  Engine.verity plus the numpy compare of the tree (inspect.verity_verify's way).
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


def spread(ts):
    """The rounds of one measurement (rates() adds the median as "ms")."""
    return {"rounds_ms": [round(x, 4) for x in ts], "spread_ms": round(max(ts) - min(ts), 4)}


def verify_device(calls, rounds, big):
    """Verify (ngpu_verity_verify_tree_device + _data_device) of an image and
    its stored tree in HBM, alternated round by round with ngpu_verity_device
    (the build) on the same bytes."""
    out = []
    s = torch.cuda.current_stream().cuda_stream
    with nydus_gpu.Engine() as eng:
        for nbytes, seed, c in ((4 * GiB, 7, calls), (16 * GiB, 9, max(2, calls // 4)))[:2 if big else 1]:
            blocks = nbytes // 512
            buf = random_device(nbytes, seed)
            lay = nydus_gpu.verity_layout(nbytes)
            tb = lay["tree_bytes"] // 4096
            d_tree = torch.full((lay["tree_bytes"],), 0xFF, dtype=torch.uint8, device="cuda")
            d_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
            d_bm = torch.full(((blocks + 63) // 64,), -1, dtype=torch.int64, device="cuda")
            d_tbm = torch.full(((tb + 63) // 64,), -1, dtype=torch.int64, device="cuda")
            d_cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            d_tcnt = torch.full((2,), -1, dtype=torch.int64, device="cuda")

            def build():
                eng.verity_device(buf.data_ptr(), nbytes, d_tree.data_ptr(), d_root.data_ptr(), stream=s)
            build()
            torch.cuda.synchronize()
            root = d_root.cpu().numpy().tobytes()

            def verify():
                eng.verity_verify_tree_device(nbytes, d_tree.data_ptr(), root, d_tbm.data_ptr(),
                                              d_tcnt.data_ptr(), stream=s)
                eng.verity_verify_data_device(buf.data_ptr(), 0, blocks, nbytes, d_tree.data_ptr(), root,
                                              d_bm.data_ptr(), d_cnt.data_ptr(), stream=s)
            verify()
            torch.cuda.synchronize()
            assert not d_bm.any() and not d_tbm.any() and not d_cnt.any() and not d_tcnt.any(), \
                "a clean image has findings"
            # what is timed does check: one flipped data byte and one flipped digest are found
            victim, slot = blocks - 12345, 777
            at = sum(level_blocks(blocks)[1:]) * 4096 + 32 * slot  # level 0's stored digest of block `slot`
            buf[victim * 512] ^= 1
            d_tree[at] ^= 1
            verify()
            torch.cuda.synchronize()
            assert d_cnt.tolist() == [2] and d_tcnt.tolist() == [1, 0], (d_cnt.tolist(), d_tcnt.tolist())
            assert d_bm[victim // 64].item() == 1 << (victim % 64) and d_bm[slot // 64].item() == 1 << (slot % 64)
            buf[victim * 512] ^= 1
            d_tree[at] ^= 1
            t = {"verify": [], "build": []}
            for _ in range(rounds):
                for name, fn in (("verify", verify), ("build", build)):
                    t[name].append(timed(fn, c))
            mv, mb = statistics.median(t["verify"]), statistics.median(t["build"])
            out.append({"measure": f"verify_device_{nbytes // GiB}GiB", "image_bytes": nbytes,
                        "tree_bytes": lay["tree_bytes"], "levels": lay["levels"], "calls_per_window": c,
                        "launches": {"verify": 2, "build": lay["levels"] + 1},
                        "verify": {**spread(t["verify"]), **rates(nbytes, mv)},
                        "build": {**spread(t["build"]), **rates(nbytes, mb)},
                        "verify_vs_build": round(mb / mv, 3)})
            eng.device_status()
            del buf, d_tree, d_bm, d_tbm
            torch.cuda.empty_cache()
    return out


def verify_host(reps):
    """Engine.verity_verify of a 2 GiB image and its tree in host memory,
    alternated with the way there was before: Engine.verity (the tree rebuilt
    and copied back) and the numpy compare of inspect.verity_verify."""
    nbytes = 2 * GiB
    data = np.random.default_rng(11).integers(0, 256, nbytes, dtype=np.uint8)
    with nydus_gpu.Engine() as eng:
        stored, info = eng.verity(data)  # warm-up: pins the two windows (kept in the engine's pool)
        root = info["root"]
        assert eng.verity_verify(data, stored, root)["bad"] == 0  # warm-up of the verify path
        t = {"verify": [], "rebuild_and_compare": []}
        for _ in range(reps):
            t0 = time.perf_counter()
            rep = eng.verity_verify(data, stored, root)
            t["verify"].append(time.perf_counter() - t0)
            assert rep["bad"] == 0 and rep["bytes"] == nbytes + stored.size
            t0 = time.perf_counter()
            tree, got = eng.verity(data)
            same = got["root"] == root and \
                not (tree.reshape(-1, 4096) != stored.reshape(-1, 4096)).any(axis=1).any()
            t["rebuild_and_compare"].append(time.perf_counter() - t0)
            assert same
        # one damaged data block: named exactly
        data[512 * 4000000 + 5] ^= 1
        rep = eng.verity_verify(data, stored, root)
        assert rep["bad"] == 1 and rep["bad_list"][0]["block"] == 4000000, rep
    row = {"measure": "verify_host_2GiB", "bytes": nbytes, "tree_bytes": int(stored.size)}
    for k, ts in t.items():
        row[k] = {"s": [round(x, 4) for x in ts], "median_s": round(statistics.median(ts), 4),
                  "spread_s": round(max(ts) - min(ts), 4),
                  "GBps_image": round(nbytes / statistics.median(ts) / 1e9, 2)}
    row["verify_vs_rebuild"] = round(statistics.median(t["rebuild_and_compare"]) / statistics.median(t["verify"]), 3)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--verify-device", action="store_true",
                    help="verify of 4 GiB and 16 GiB images in HBM, alternated with the build")
    ap.add_argument("--verify-host", action="store_true",
                    help="Engine.verity_verify of 2 GiB in host memory against rebuild-and-compare")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-16g", action="store_true", help="--device: skip the 16 GiB image")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("verity_bench: no GPU (there is no CPU fallback)")
    if args.verify_device:
        for r in verify_device(args.calls, args.rounds, not args.no_16g):
            print(json.dumps(r), flush=True)
    if args.verify_host:
        for r in verify_host(args.reps):
            print(json.dumps(r), flush=True)
    if args.verify_device or args.verify_host:
        return
    if args.device or not args.host:
        for r in device_stage(args.calls, args.rounds, not args.no_16g):
            print(json.dumps(r), flush=True)
    if args.host or not args.device:
        for r in host_pipeline(args.reps):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
