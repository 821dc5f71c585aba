#!/usr/bin/env python3
"""Node dict remode in both directions, on one GPU listed W times, next to its
floor and to what it replaces.  The dict holds m sha256-sized random entries in 10
blobs (blob = position * 10 // m) with placement rows.  Alternated, `rounds` times
each after one warm-up round:

  split      Node.dict_remode(replicated, PARTITION | COPY): wall time of the call
             and, per part, the device time between HIP events on its build stream
             (NGPU_DICT_TRACE lines: keep + scan, compact + build); the slowest part
             is reported, and the host's time per phase of the call
  join       Node.dict_remode(partitioned, REPLICATE): the same with its phases
             (bounds, copies + scatter, build), at the default window
  floor      ChunkDict.retire([]) (ngpu_dict_retire with n == 0) of ONE plain dict
             holding what one GPU ends up with: part 0's m / W rows for the split, all
             m rows for the join -- the copy and table build of the same rows with no
             cross-part work and the GPU to itself
  yardstick  what a caller had to do before: Node.dict_export_parts, then
             Node.dict_create in the other mode (wall time, and each leg)

One GPU listed W times says nothing about xGMI: every peer copy here stays inside
one HBM, and the W parts' kernels share one GPU's bandwidth.  On W distinct GPUs a
join moves (W - 1) / W x m x 64 B over the links into every replica.

usage: tools/node_dict_remode_bench.py [WS] [SIZES_M] [ROUNDS] [YARDSTICK_ROUNDS]
       defaults: 2,8  1,16  5  3        -> JSON lines"""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first traces a dict call

from dict_extend_bench import Stderr, spread  # noqa: E402

NB = 10
SPLIT_LINE = (r"ngpu node_dict_remode split part=(\d+) m=\d+ s_o=(\d+) device_us=([0-9.]+) "
              r"keep_scan_us=([0-9.]+) compact_build_us=([0-9.]+)")
JOIN_LINE = (r"ngpu node_dict_remode join part=(\d+) m=\d+ m_o=(\d+) windows=(\d+) device_us=([0-9.]+) "
             r"bounds_us=([0-9.]+) copy_scatter_us=([0-9.]+) build_us=([0-9.]+)")
HOST_LINE = (r"ngpu node_dict_remode (?:split|join) host W=\d+ m=\d+ enqueue_ms=([0-9.]+) wait_ms=([0-9.]+) "
             r"alloc_launch_ms=([0-9.]+) place_wait_ms=([0-9.]+) release_ms=([0-9.]+)")
HOST_KEYS = ("enqueue_ms", "wait_ms", "alloc_launch_ms", "place_wait_ms", "release_ms")
PLAIN_LINE = r"ngpu dict_retire m=(\d+) s=(\d+) device_us=([0-9.]+) keep_scan_us=([0-9.]+) compact_build_us=([0-9.]+)"
SPLIT_NAMES = ("wall_ms", "device_us", "keep_scan_us", "compact_build_us")
JOIN_NAMES = ("wall_ms", "device_us", "bounds_us", "copy_scatter_us", "build_us")
FLOOR_NAMES = ("wall_ms", "device_us", "keep_scan_us", "compact_build_us")


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import rafs
    ws = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "2,8").split(",")]
    sizes = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,16").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    yard_rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    err = Stderr()
    g = torch.Generator(device="cuda").manual_seed(0x4E0D)
    part_mode = nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY
    rep_mode = nydus_gpu.NODE_DICT_REPLICATE
    host = []  # the last call's host phases (HOST_KEYS), when it printed them

    def timed(fn, pattern):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        text = err.take()
        host[:] = [float(x) for x in (re.findall(HOST_LINE, text) or [()])[-1]]
        return out, wall, re.findall(pattern, text)

    def yardstick(node, base, mode, m):
        t0 = time.perf_counter()
        recs, _ = node.dict_export_parts(base)
        t1 = time.perf_counter()
        c = node.dict_create(recs, mode=mode)
        t2 = time.perf_counter()
        assert c.entries == m
        c.release()
        return ((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3)

    try:
        for mm in sizes:
            m = mm * 1_000_000
            dd = torch.empty((m, 32), dtype=torch.uint8, device="cuda")
            dd.random_(0, 256, generator=g)
            h_all = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
            h_all["block_id"] = dd.cpu().numpy()
            del dd
            torch.cuda.empty_cache()
            h_all["blob_index"] = np.arange(m, dtype=np.int64) * NB // m
            h_all["uncompressed_size"] = 1 << 20
            h_all["compressed_size"] = 1 << 19
            h_all["compressed_offset"] = np.arange(m, dtype=np.uint64) << 19
            h_all["index"] = np.arange(m, dtype=np.uint32)
            for W in ws:
                node = nydus_gpu.Node([0] * W, digester="sha256")
                try:
                    dg = h_all["block_id"]
                    owner = (((dg[:, 0].astype(np.uint32) << 8) | dg[:, 1]) * W) >> 16
                    share = h_all[owner == 0]
                    rep = node.dict_create(h_all, mode=rep_mode)
                    part = node.dict_create(h_all, mode=part_mode)
                    one_share = node.engines[0].dict_create(share)
                    one_all = node.engines[0].dict_create(h_all)
                    res = {"split": [], "join": [], "floor_split": [], "floor_join": [], "yard_split": [],
                           "yard_join": []}
                    for r in range(-1, rounds):  # round -1 warms every path up and is not kept
                        out, wall, t = timed(lambda: node.dict_remode(rep, part_mode), SPLIT_LINE)
                        assert out.entries == m and len(t) == W and sum(int(x[1]) for x in t) == m, t
                        out.release()
                        assert len(host) == len(HOST_KEYS), host
                        res["split"].append((wall,) + tuple(max(float(x[i]) for x in t) for i in (2, 3, 4)) +
                                            tuple(host))
                        out, wall, t = timed(lambda: node.dict_remode(part, rep_mode), JOIN_LINE)
                        assert out.entries == m and len(t) == W and sum(int(x[1]) for x in t) == m, t
                        out.release()
                        assert len(host) == len(HOST_KEYS), host
                        res["join"].append((wall,) + tuple(max(float(x[i]) for x in t) for i in (3, 4, 5, 6)) +
                                           tuple(host))
                        for key, one, want in (("floor_split", one_share, len(share)), ("floor_join", one_all, m)):
                            out, wall, t = timed(lambda: one.retire([]), PLAIN_LINE)
                            assert out.entries == want == int(t[-1][1]), (out.entries, want, t)
                            out.release()
                            res[key].append((wall,) + tuple(float(x) for x in t[-1][2:]))
                        if r < yard_rounds:
                            res["yard_split"].append(yardstick(node, rep, part_mode, m))
                            res["yard_join"].append(yardstick(node, part, rep_mode, m))
                        if r < 0:
                            for v in res.values():
                                v.clear()
                            continue
                        s, j = res["split"][-1], res["join"][-1]
                        line = {"W": W, "dict_entries": m, "round": r,
                                **{f"split_{n}": round(s[i], 3) for i, n in enumerate(SPLIT_NAMES)},
                                "split_host_ms": dict(zip(HOST_KEYS, s[len(SPLIT_NAMES):])),
                                **{f"join_{n}": round(j[i], 3) for i, n in enumerate(JOIN_NAMES)},
                                "join_host_ms": dict(zip(HOST_KEYS, j[len(JOIN_NAMES):])),
                                "floor_split_entries": len(share),
                                **{f"floor_split_{n}": round(res["floor_split"][-1][i], 3)
                                   for i, n in enumerate(FLOOR_NAMES)},
                                **{f"floor_join_{n}": round(res["floor_join"][-1][i], 3)
                                   for i, n in enumerate(FLOOR_NAMES)}}
                        if len(res["yard_split"]) > r:
                            for k in ("yard_split", "yard_join"):
                                y = res[k][r]
                                line.update({f"{k}_wall_ms": round(y[0], 3), f"{k}_export_ms": round(y[1], 3),
                                             f"{k}_create_ms": round(y[2], 3)})
                        print(json.dumps(line), flush=True)
                    summ = {f"split_{n}": spread([x[i] for x in res["split"]]) for i, n in enumerate(SPLIT_NAMES)}
                    summ["split_host_ms"] = {k: spread([x[len(SPLIT_NAMES) + i] for x in res["split"]])
                                             for i, k in enumerate(HOST_KEYS)}
                    summ.update({f"join_{n}": spread([x[i] for x in res["join"]]) for i, n in enumerate(JOIN_NAMES)})
                    summ["join_host_ms"] = {k: spread([x[len(JOIN_NAMES) + i] for x in res["join"]])
                                            for i, k in enumerate(HOST_KEYS)}
                    for key in ("floor_split", "floor_join"):
                        summ.update({f"{key}_{n}": spread([x[i] for x in res[key]]) for i, n in enumerate(FLOOR_NAMES)})
                    for key in ("yard_split", "yard_join"):
                        if res[key]:
                            for i, n in enumerate(("wall_ms", "export_ms", "create_ms")):
                                summ[f"{key}_{n}"] = spread([x[i] for x in res[key]])
                    print(json.dumps({"W": W, "dict_entries": m, "floor_split_entries": len(share),
                                      "join_peer_bytes_per_replica": (W - 1) * m * 64 // W, "summary": summ}),
                          flush=True)
                    for h in (one_all, one_share, part, rep):
                        h.release()
                finally:
                    node.close()
            del h_all
    finally:
        err.close()


if __name__ == "__main__":
    main()
