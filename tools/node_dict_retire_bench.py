#!/usr/bin/env python3
"""Retire of a partitioned node dict across its parts, on one GPU listed W times
(copy exchange), next to its floor and to what it replaces.  The dict holds m
entries in 10 blobs, blob = position % 10 (every keep word is mixed), with
placement rows; retiring 1 blob drops 10 % of the records, 5 blobs 50 %.
Alternated, `rounds` times each after one warm-up round:

  retire_parts  Node.dict_retire_parts (ngpu_node_dict_retire_parts): wall time of
                the call and, per part, the device time between HIP events on its
                build stream (NGPU_DICT_TRACE lines: keep + local scan, gather +
                merge + global scan, compact + build); the slowest part is reported,
                and the host's time per phase of the call from the same trace
  floor         ChunkDict.retire (ngpu_dict_retire) of ONE plain dict holding part
                0's share of the same rows: what a part's compaction costs with no
                cross-part work at all
  create        what a user had to do before: Node.dict_create over the surviving
                host records

One GPU listed W times says nothing about xGMI: every peer copy here stays inside
one HBM, and the W parts' kernels share one GPU's bandwidth.

usage: tools/node_dict_retire_bench.py [WS] [SIZES_M] [PERCENTS] [ROUNDS] [CREATE_ROUNDS]
       defaults: 2,8  1,16  10,50  5  3        -> JSON lines (200 in SIZES_M if HBM and host memory allow)"""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first retires a dict

from dict_extend_bench import Stderr, spread  # noqa: E402

NB = 10
GONE = {10: [3], 50: [1, 3, 5, 7, 9]}
PART_LINE = (r"ngpu node_dict_retire_parts part=(\d+) m=\d+ m_o=(\d+) s_o=(\d+) device_us=([0-9.]+) "
             r"keep_scan_us=([0-9.]+) gather_merge_us=([0-9.]+) compact_build_us=([0-9.]+)")
HOST_LINE = (r"ngpu node_dict_retire_parts host W=\d+ m=\d+ enqueue_ms=([0-9.]+) wait_ms=([0-9.]+) "
             r"alloc_launch_ms=([0-9.]+) place_wait_ms=([0-9.]+) release_ms=([0-9.]+)")
HOST_KEYS = ("enqueue_ms", "wait_ms", "alloc_launch_ms", "place_wait_ms", "release_ms")
PLAIN_LINE = r"ngpu dict_retire m=(\d+) s=(\d+) device_us=([0-9.]+) keep_scan_us=([0-9.]+) compact_build_us=([0-9.]+)"


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import rafs
    ws = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "2,8").split(",")]
    sizes = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "1,16").split(",")]
    pcts = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "10,50").split(",")]
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    create_rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 3
    err = Stderr()
    g = torch.Generator(device="cuda").manual_seed(0x9E71)

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
            d_recs = torch.zeros((m, 80), dtype=torch.uint8, device="cuda")
            d_recs[:, :32].random_(0, 256, generator=g)
            h_all = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
            torch.from_numpy(h_all.view(np.uint8).reshape(m, 80)).copy_(d_recs)
            del d_recs
            torch.cuda.empty_cache()
            h_all["blob_index"] = np.arange(m) % NB
            h_all["uncompressed_size"] = h_all["compressed_size"] = 1 << 20
            h_all["index"] = np.arange(m, dtype=np.uint32)
            for W in ws:
                node = nydus_gpu.Node([0] * W, digester="sha256")
                try:
                    d = h_all["block_id"]
                    owner = (((d[:, 0].astype(np.uint32) << 8) | d[:, 1]) * W) >> 16
                    share = h_all[owner == 0]
                    base = node.dict_create(h_all, mode=nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY)
                    one = node.engines[0].dict_create(share)
                    for pct in pcts:
                        gone = GONE[pct]
                        remap = np.cumsum(~np.isin(np.arange(NB), gone)) - 1
                        survivors = h_all[~np.isin(h_all["blob_index"], gone)]
                        survivors["blob_index"] = remap[survivors["blob_index"]]
                        s = len(survivors)
                        s_share = int((~np.isin(share["blob_index"], gone)).sum())
                        res = {"parts": [], "floor": [], "create": []}
                        for r in range(-1, rounds):  # round -1 warms every path up and is not kept
                            out, wall, t = timed(lambda: node.dict_retire_parts(base, gone), PART_LINE)
                            assert out.entries == s and len(t) == W, (out.entries, s, t)
                            assert sum(int(x[2]) for x in t) == s
                            out.release()
                            assert len(host) == len(HOST_KEYS), host
                            res["parts"].append((wall,) + tuple(max(float(x[i]) for x in t) for i in (3, 4, 5, 6)) +
                                                tuple(host))
                            out, wall, t = timed(lambda: one.retire(gone), PLAIN_LINE)
                            assert out.entries == s_share == int(t[-1][1]), (out.entries, s_share, t)
                            out.release()
                            res["floor"].append((wall, float(t[-1][2]), float(t[-1][3]), float(t[-1][4])))
                            if r < create_rounds:
                                out, wall, _ = timed(lambda: node.dict_create(
                                    survivors, mode=nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY), PART_LINE)
                                assert out.entries == s
                                out.release()
                                res["create"].append((wall,))
                            if r < 0:
                                for v in res.values():
                                    v.clear()
                                continue
                            p, f = res["parts"][-1], res["floor"][-1]
                            print(json.dumps({"W": W, "dict_entries": m, "retired_percent": pct, "survivors": s,
                                              "round": r, "retire_parts_wall_ms": round(p[0], 3),
                                              "retire_parts_device_us": p[1], "retire_parts_keep_scan_us": p[2],
                                              "retire_parts_gather_merge_us": p[3],
                                              "retire_parts_compact_build_us": p[4],
                                              "retire_parts_host_ms": dict(zip(HOST_KEYS, p[5:])),
                                              "floor_entries": len(share), "floor_wall_ms": round(f[0], 3),
                                              "floor_device_us": f[1], "floor_keep_scan_us": f[2],
                                              "floor_compact_build_us": f[3],
                                              **({"create_wall_ms": round(res["create"][-1][0], 3)}
                                                 if len(res["create"]) > r else {})}), flush=True)
                        names = ("wall_ms", "device_us", "keep_scan_us", "gather_merge_us", "compact_build_us")
                        summ = {f"retire_parts_{n}": spread([x[i] for x in res["parts"]]) for i, n in enumerate(names)}
                        summ["retire_parts_host_ms"] = {k: spread([x[5 + i] for x in res["parts"]])
                                                        for i, k in enumerate(HOST_KEYS)}
                        fn = ("wall_ms", "device_us", "keep_scan_us", "compact_build_us")
                        summ.update({f"floor_{n}": spread([x[i] for x in res["floor"]]) for i, n in enumerate(fn)})
                        summ["create_wall_ms"] = spread([x[0] for x in res["create"]])
                        ratio = summ["retire_parts_device_us"]["median"] / summ["floor_device_us"]["median"]
                        print(json.dumps({"W": W, "dict_entries": m, "retired_percent": pct, "survivors": s,
                                          "floor_entries": len(share), "summary": summ,
                                          "device_ratio_to_floor": round(ratio, 2)}), flush=True)
                        del survivors
                    one.release()
                    base.release()
                finally:
                    node.close()
            del h_all
    finally:
        err.close()


if __name__ == "__main__":
    main()
