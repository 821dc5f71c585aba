#!/usr/bin/env python3
"""Distill of a partitioned node dict across its parts, on one GPU listed W times
(copy exchange), next to its floor and to what it replaces.  The dict holds m
sha256-sized entries in 10 blobs (blob = position * 10 // m) with placement rows:
the first m (1 - f) rows are distinct, every later row repeats a random one of
them (f = the shadow fraction).  Alternated, `rounds` times each after one warm-up
round:

  distill_parts  Node.dict_distill_parts (ngpu_node_dict_distill_parts): wall time
                 of the call and, per part, the device time between HIP events on
                 its build stream (NGPU_DICT_TRACE lines: count, keep + local scan,
                 gather + merge + global scan, compact + build); the slowest part is
                 reported, and the host's time per phase of the call from the same
                 trace
  floor          ChunkDict.distill (ngpu_dict_distill) of ONE plain dict holding
                 part 0's share of the same rows: what a part's work costs with no
                 cross-part step and the GPU to itself
  host           what a user had to do before: Node.dict_export_parts, the first
                 row per digest in numpy (tools/dict_distill_bench.py's
                 host_distill), Node.dict_create over the survivors

One GPU listed W times says nothing about xGMI: every peer copy here stays inside
one HBM, and the W parts' kernels share one GPU's bandwidth.

usage: tools/node_dict_distill_bench.py [WS] [SIZES_M] [SHADOW_PERCENTS] [ROUNDS] [HOST_ROUNDS]
       defaults: 2,8  1,16  0,50,90  5  3        -> JSON lines"""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first distils a dict

from dict_distill_bench import host_distill  # noqa: E402
from dict_extend_bench import Stderr, spread  # noqa: E402

NB = 10
PART_LINE = (r"ngpu node_dict_distill_parts part=(\d+) m=\d+ m_o=(\d+) s_o=(\d+) device_us=([0-9.]+) "
             r"count_us=([0-9.]+) keep_scan_us=([0-9.]+) gather_merge_us=([0-9.]+) compact_build_us=([0-9.]+)")
HOST_LINE = (r"ngpu node_dict_distill_parts host W=\d+ m=\d+ enqueue_ms=([0-9.]+) wait_ms=([0-9.]+) "
             r"alloc_launch_ms=([0-9.]+) place_wait_ms=([0-9.]+) release_ms=([0-9.]+)")
HOST_KEYS = ("enqueue_ms", "wait_ms", "alloc_launch_ms", "place_wait_ms", "release_ms")
PLAIN_LINE = (r"ngpu dict_distill m=(\d+) s=(\d+) device_us=([0-9.]+) count_us=([0-9.]+) "
              r"keep_scan_us=([0-9.]+) compact_build_us=([0-9.]+)")
PART_NAMES = ("wall_ms", "device_us", "count_us", "keep_scan_us", "gather_merge_us", "compact_build_us")
FLOOR_NAMES = ("wall_ms", "device_us", "count_us", "keep_scan_us", "compact_build_us")


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import rafs
    ws = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "2,8").split(",")]
    sizes = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,16").split(",")]
    pcts = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "0,50,90").split(",")]
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    host_rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    err = Stderr()
    g = torch.Generator(device="cuda").manual_seed(0xD157)
    mode = nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY

    host = []  # the last call's host phases (HOST_KEYS), when it printed them

    def timed(fn, pattern):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        text = err.take()
        host[:] = [float(x) for x in (re.findall(HOST_LINE, text) or [()])[-1]]
        return out, wall, re.findall(pattern, text)

    try:
        for mm in sizes:
            m = mm * 1_000_000
            for pct in pcts:
                d = m - m * pct // 100
                dd = torch.empty((m, 32), dtype=torch.uint8, device="cuda")
                dd[:d].random_(0, 256, generator=g)
                if d < m:
                    src = torch.randint(0, d, (m - d,), generator=g, device="cuda")
                    dd[d:] = dd[:d][src]
                    del src
                h_all = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
                h_all["block_id"] = dd.cpu().numpy()
                del dd
                torch.cuda.empty_cache()
                h_all["blob_index"] = np.arange(m, dtype=np.int64) * NB // m
                h_all["uncompressed_size"] = h_all["compressed_size"] = 1 << 20
                h_all["index"] = np.arange(m, dtype=np.uint32)
                for W in ws:
                    node = nydus_gpu.Node([0] * W, digester="sha256")
                    try:
                        dg = h_all["block_id"]
                        owner = (((dg[:, 0].astype(np.uint32) << 8) | dg[:, 1]) * W) >> 16
                        share = h_all[owner == 0]
                        d_share = len(np.unique(np.ascontiguousarray(share["block_id"][:, :8]).view("<u8")[:, 0]))
                        base = node.dict_create(h_all, mode=mode)
                        one = node.engines[0].dict_create(share)
                        res = {"parts": [], "floor": [], "host": []}
                        for r in range(-1, rounds):  # round -1 warms every path up and is not kept
                            (out, info), wall, t = timed(lambda: node.dict_distill_parts(base, 1), PART_LINE)
                            assert out.entries == d == info["distinct"] and len(t) == W, (out.entries, d, t)
                            assert sum(int(x[2]) for x in t) == d
                            out.release()
                            assert len(host) == len(HOST_KEYS), host
                            res["parts"].append((wall,) + tuple(max(float(x[i]) for x in t) for i in (3, 4, 5, 6, 7)) +
                                                tuple(host))
                            (out, _), wall, t = timed(lambda: one.distill(1), PLAIN_LINE)
                            assert out.entries == d_share == int(t[-1][1]), (out.entries, d_share, t)
                            out.release()
                            res["floor"].append((wall,) + tuple(float(x) for x in t[-1][2:]))
                            if r < host_rounds:
                                t0 = time.perf_counter()
                                recs, _ = node.dict_export_parts(base)
                                t1 = time.perf_counter()
                                kept, _ = host_distill(np, recs)
                                t2 = time.perf_counter()
                                c = node.dict_create(kept, mode=mode)
                                t3 = time.perf_counter()
                                assert c.entries == d
                                c.release()
                                del recs, kept
                                res["host"].append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
                            if r < 0:
                                for v in res.values():
                                    v.clear()
                                continue
                            p, f = res["parts"][-1], res["floor"][-1]
                            line = {"W": W, "dict_entries": m, "shadow_percent": pct, "distinct": d, "round": r,
                                    **{f"distill_parts_{n}": round(p[i], 3) for i, n in enumerate(PART_NAMES)},
                                    "distill_parts_host_ms": dict(zip(HOST_KEYS, p[len(PART_NAMES):])),
                                    "floor_entries": len(share),
                                    **{f"floor_{n}": round(f[i], 3) for i, n in enumerate(FLOOR_NAMES)}}
                            if len(res["host"]) > r:
                                h = res["host"][r]
                                line.update(host_wall_ms=round(h[0], 3), host_export_ms=round(h[1], 3),
                                            host_numpy_ms=round(h[2], 3), host_create_ms=round(h[3], 3))
                            print(json.dumps(line), flush=True)
                        summ = {f"distill_parts_{n}": spread([x[i] for x in res["parts"]])
                                for i, n in enumerate(PART_NAMES)}
                        summ["distill_parts_host_ms"] = {k: spread([x[len(PART_NAMES) + i] for x in res["parts"]])
                                                         for i, k in enumerate(HOST_KEYS)}
                        summ.update({f"floor_{n}": spread([x[i] for x in res["floor"]])
                                     for i, n in enumerate(FLOOR_NAMES)})
                        if res["host"]:
                            for i, n in enumerate(("wall_ms", "export_ms", "numpy_ms", "create_ms")):
                                summ[f"host_{n}"] = spread([x[i] for x in res["host"]])
                        ratio = summ["distill_parts_device_us"]["median"] / summ["floor_device_us"]["median"]
                        print(json.dumps({"W": W, "dict_entries": m, "shadow_percent": pct, "distinct": d,
                                          "floor_entries": len(share), "summary": summ,
                                          "device_ratio_to_floor": round(ratio, 2)}), flush=True)
                        one.release()
                        base.release()
                    finally:
                        node.close()
                del h_all
    finally:
        err.close()


if __name__ == "__main__":
    main()
