#!/usr/bin/env python3
"""Dict distill by dict size and shadow fraction: what does keeping one row per
digest of a dict of m entries cost on the GPU (ngpu_dict_distill: the counting
pass through the table, keep bits with the counters, their scan, the compaction,
the table build), next to

  - a retire of nothing (ngpu_dict_retire, n == 0) on the same dict: the same
    compaction and table build over m survivors without the counting pass, and
  - the host path: ChunkDict.export, the first row per digest and its count in
    numpy (a stable argsort of the first 8 digest bytes; the digests are random),
    Engine.dict_create over the survivors.

For each m a base of m sha256-sized digests in 10 blobs is created from device
arrays: the first m (1 - f) rows are distinct, every later row repeats a random
one of them (f = the shadow fraction), as a dict folded from layers that reuse
its chunks does.  "one" is the dict whose m rows all hold one digest (every add
of the counting pass lands on one word), measured next to the all-distinct dict
(f = 0) of the same size.  Wall time is the call; device time comes from the
library's NGPU_DICT_TRACE lines (HIP events on its build stream).

usage: tools/dict_distill_bench.py [SIZES_M] [SHADOW_PERCENTS] [ROUNDS] [HOST_PATH_UP_TO_M]
       defaults: 1,16,max  0,50,90,one  5  16  -> JSON lines
       "max": the largest dict that fits next to its distilled copy (at most 1,000 M
       rows; the host path is left out above HOST_PATH_UP_TO_M)"""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first distils / retires a dict

from dict_extend_bench import Stderr, spread  # noqa: E402

NB = 10
# HBM per row while a distill runs: the base (64-B record, up to 32 B of table), the
# result with a fork's room (1.5 x that), 4 B of counts, and the arrays the base was made from
BYTES_PER_ROW = 96 + 144 + 8 + 44
DISTILL_RE = (r"ngpu dict_distill m=\d+ s=(\d+) device_us=([0-9.]+) count_us=([0-9.]+) "
              r"keep_scan_us=([0-9.]+) compact_build_us=([0-9.]+)")
RETIRE_RE = (r"ngpu dict_retire m=\d+ s=(\d+) device_us=([0-9.]+) keep_scan_us=([0-9.]+) "
             r"compact_build_us=([0-9.]+)")


def host_distill(np, recs):
    """The first row of every digest, in table order, and the largest count."""
    key = np.ascontiguousarray(recs["block_id"][:, :8]).view("<u8")[:, 0]
    order = np.argsort(key, kind="stable")
    k = key[order]
    head = np.ones(len(k), bool)
    head[1:] = k[1:] != k[:-1]
    first = np.sort(order[head])
    counts = np.diff(np.append(np.flatnonzero(head), len(k)))
    return recs[first], int(counts.max()) if len(k) else 0


def main():
    import numpy as np
    import torch
    import nydus_gpu
    sizes = (sys.argv[1] if len(sys.argv) > 1 else "1,16,max").split(",")
    fracs = (sys.argv[2] if len(sys.argv) > 2 else "0,50,90,one").split(",")
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    host_up_to = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    err = Stderr()
    eng = nydus_gpu.Engine(device=0, digester="sha256")
    g = torch.Generator(device="cuda").manual_seed(0xD157)

    def timed(fn, pattern):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        got = re.findall(pattern, err.take())
        return out, wall, got[-1] if got else None

    try:
        for size in sizes:
            if size == "max":
                free, _ = torch.cuda.mem_get_info()
                m = min(free // BYTES_PER_ROW // 1_000_000, 1000) * 1_000_000
            else:
                m = int(size) * 1_000_000
            for frac in fracs:
                d = 1 if frac == "one" else m - m * int(frac) // 100
                dd = torch.empty((m, 32), dtype=torch.uint8, device="cuda")
                dd[:d].random_(0, 256, generator=g)
                if d < m:
                    src = torch.randint(0, d, (m - d,), generator=g, device="cuda")
                    dd[d:] = dd[:d][src]
                    del src
                pos = torch.arange(m, dtype=torch.int64, device="cuda")
                bl = (pos * NB // m).to(torch.int32)
                ix = pos.to(torch.int32)
                del pos
                us = torch.full((m,), 1 << 20, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()  # the build reads the arrays from its own stream
                base, create_wall, _ = timed(
                    lambda: eng.dict_create_device(dd.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), m, NB),
                    r"$^")
                del dd, us, ix, bl
                torch.cuda.empty_cache()
                res = {"distill": [], "retire": [], "host": []}
                host = m <= host_up_to * 1_000_000
                info = None
                for r in range(rounds):
                    (out, info), wall, t = timed(lambda: base.distill(1), DISTILL_RE)
                    assert out.entries == d == int(t[0]) == info["distinct"], (out.entries, d, t)
                    out.release()
                    res["distill"].append((wall,) + tuple(float(x) for x in t[1:]))
                    out, wall, t = timed(lambda: base.retire([]), RETIRE_RE)
                    assert out.entries == m == int(t[0])
                    out.release()
                    res["retire"].append((wall,) + tuple(float(x) for x in t[1:]))
                    line = {"dict_entries": m, "shadow": frac, "distinct": d, "round": r,
                            "distill_wall_ms": round(res["distill"][-1][0], 3),
                            "distill_device_us": res["distill"][-1][1],
                            "distill_count_us": res["distill"][-1][2],
                            "distill_keep_scan_us": res["distill"][-1][3],
                            "distill_compact_build_us": res["distill"][-1][4],
                            "retire_nothing_wall_ms": round(res["retire"][-1][0], 3),
                            "retire_nothing_device_us": res["retire"][-1][1],
                            "retire_nothing_keep_scan_us": res["retire"][-1][2],
                            "retire_nothing_compact_build_us": res["retire"][-1][3]}
                    if host and (r == 0 or m <= 1_000_000):
                        t0 = time.perf_counter()
                        recs, _ = base.export()
                        t1 = time.perf_counter()
                        kept, most = host_distill(np, recs)
                        t2 = time.perf_counter()
                        c = eng.dict_create(kept)
                        t3 = time.perf_counter()
                        assert c.entries == d and most == info["max_refs"], (c.entries, d, most, info["max_refs"])
                        c.release()
                        del recs, kept
                        res["host"].append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
                        line.update(host_wall_ms=round(res["host"][-1][0], 3), host_export_ms=round(res["host"][-1][1], 3),
                                    host_numpy_ms=round(res["host"][-1][2], 3), host_create_ms=round(res["host"][-1][3], 3))
                    print(json.dumps(line), flush=True)
                summary = {"base_create_wall_ms": round(create_wall, 3), "max_refs": info["max_refs"] if info else 0,
                           "distill_device_us": spread([x[1] for x in res["distill"]]),
                           "distill_count_us": spread([x[2] for x in res["distill"]]),
                           "distill_keep_scan_us": spread([x[3] for x in res["distill"]]),
                           "distill_compact_build_us": spread([x[4] for x in res["distill"]]),
                           "distill_wall_ms": spread([x[0] for x in res["distill"]]),
                           "retire_nothing_device_us": spread([x[1] for x in res["retire"]]),
                           "retire_nothing_wall_ms": spread([x[0] for x in res["retire"]])}
                if res["host"]:
                    summary["host_wall_ms"] = spread([x[0] for x in res["host"]])
                    summary["host_export_ms"] = spread([x[1] for x in res["host"]])
                    summary["host_numpy_ms"] = spread([x[2] for x in res["host"]])
                    summary["host_create_ms"] = spread([x[3] for x in res["host"]])
                print(json.dumps({"dict_entries": m, "shadow": frac, "distinct": d, "summary": summary}), flush=True)
                base.release()
    finally:
        eng.close()
        err.close()


if __name__ == "__main__":
    main()
