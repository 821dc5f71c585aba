#!/usr/bin/env python3
"""Dict retire by dict size: what does dropping the records of some blobs from a
dict of m entries cost on the GPU (ngpu_dict_retire: keep bits, their scan, the
compaction, the table build), next to the fork of an extend of the same base
(the same traffic class: a device-to-device copy of m records and a table build)
and next to ngpu_dict_create over the surviving records in host memory (the only
way to retire without it)?

For each m a base of m random sha256-sized digests in 10 blobs is created from
device arrays.  layout "runs": blob = position * 10 / m (a dict grown layer by
layer: every keep word is all ones or all zeros); "mixed": blob = position % 10
(every keep word is mixed).  Retiring 1 blob drops 10 % of the records, 5 blobs
50 %.  Then, alternated, `rounds` times each: the retire, a fork of the base by
128 records, and ngpu_dict_create over the survivors.  Wall time is the call;
device time comes from the library's NGPU_DICT_TRACE lines (HIP events on its
build stream).

usage: tools/dict_retire_bench.py [SIZES_M] [PERCENTS] [ROUNDS] [CREATE_ROUNDS_AT_200M] [LAYOUTS]
       defaults: 1,16,200  10,50  5  3  runs,mixed (mixed only below 100M)  -> JSON lines"""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first extends / retires a dict

from dict_extend_bench import Stderr, spread  # noqa: E402

NB = 10
GONE = {10: [3], 50: [1, 3, 5, 7, 9]}


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import rafs
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,16,200").split(",")]
    pcts = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "10,50").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    big_rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    layouts = (sys.argv[5] if len(sys.argv) > 5 else "runs,mixed").split(",")
    err = Stderr()
    eng = nydus_gpu.Engine(device=0, digester="sha256")
    g = torch.Generator(device="cuda").manual_seed(0xD1C7)
    rng = np.random.default_rng(0xD1C7)
    extra = np.zeros(128, rafs.CHUNK_INFO_DTYPE)
    extra["block_id"] = rng.integers(0, 256, (128, 32), dtype=np.uint8)
    extra["uncompressed_size"] = 1 << 20

    def timed(fn, pattern):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        got = re.findall(pattern, err.take())
        return out, wall, got[-1] if got else None

    try:
        for mm in sizes:
            m = mm * 1_000_000
            for layout in layouts:
                if layout == "mixed" and mm >= 100:
                    continue
                d_recs = torch.empty((m, 80), dtype=torch.uint8, device="cuda")
                d_recs.random_(0, 256, generator=g)
                pos = torch.arange(m, dtype=torch.int64, device="cuda")
                bl = (pos * NB // m if layout == "runs" else pos % NB).to(torch.int32)
                d_recs[:, 32:36] = bl.view(torch.uint8).reshape(m, 4)
                h_all = np.zeros((m, 80), np.uint8)
                torch.from_numpy(h_all).copy_(d_recs)
                dd = d_recs[:, :32].contiguous()
                del d_recs, pos
                us = torch.full((m,), 1 << 20, dtype=torch.int32, device="cuda")
                ix = torch.arange(m, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()  # the build reads the arrays from its own stream
                base = eng.dict_create_device(dd.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), m, NB)
                del dd, us, ix
                h_blob = bl.cpu().numpy()
                del bl
                torch.cuda.empty_cache()
                # the same rows WITH host placement rows (a dict from 80-B records keeps them): its
                # retire also brings the keep words back and compacts those rows on the host
                placed = eng.dict_create(h_all)
                for pct in pcts:
                    gone = GONE[pct]
                    keep = ~np.isin(h_blob, gone)
                    survivors = h_all[keep]  # what a host rebuild uploads (blob indices renumbered)
                    remap = np.cumsum(~np.isin(np.arange(NB), gone)) - 1
                    survivors[:, 32:36] = remap[h_blob[keep]].astype("<u4").view(np.uint8).reshape(-1, 4)
                    s = len(survivors)
                    res = {"retire": [], "placed": [], "fork": [], "create": []}
                    n_create = big_rounds if mm >= 100 else rounds
                    for r in range(rounds):
                        out, wall, t = timed(lambda: base.retire(gone),
                                             r"ngpu dict_retire m=\d+ s=(\d+) device_us=([0-9.]+) "
                                             r"keep_scan_us=([0-9.]+) compact_build_us=([0-9.]+)")
                        assert out.entries == s == int(t[0]), (out.entries, s, t)
                        out.release()
                        res["retire"].append((wall, float(t[1]), float(t[2]), float(t[3])))
                        out, wall, t = timed(lambda: placed.retire(gone), r"ngpu dict_retire m=\d+ s=(\d+) ")
                        assert out.entries == s
                        out.release()
                        res["placed"].append((wall, None))
                        f, wall, t = timed(lambda: base.extend(extra),
                                           r"ngpu dict_extend (\w+) m=\d+ k=\d+ device_us=([0-9.]+)")
                        assert t[0] == "fork" and f.entries == m + 128
                        f.release()
                        res["fork"].append((wall, float(t[1])))
                        if r < n_create:
                            c, wall, _ = timed(lambda: eng.dict_create(survivors), r"$^")
                            assert c.entries == s
                            c.release()
                            res["create"].append((wall, None))
                        print(json.dumps({"dict_entries": m, "layout": layout, "retired_percent": pct,
                                          "survivors": s, "round": r,
                                          "retire_wall_ms": round(res["retire"][-1][0], 3),
                                          "retire_device_us": res["retire"][-1][1],
                                          "retire_keep_scan_us": res["retire"][-1][2],
                                          "retire_compact_build_us": res["retire"][-1][3],
                                          "retire_with_placement_rows_wall_ms": round(res["placed"][-1][0], 3),
                                          "fork_wall_ms": round(res["fork"][-1][0], 3),
                                          "fork_device_us": res["fork"][-1][1],
                                          **({"create_wall_ms": round(res["create"][-1][0], 3)}
                                             if len(res["create"]) > r else {})}), flush=True)
                    print(json.dumps({"dict_entries": m, "layout": layout, "retired_percent": pct,
                                      "survivors": s, "summary": {
                        "retire_device_us": spread([x[1] for x in res["retire"]]),
                        "retire_keep_scan_us": spread([x[2] for x in res["retire"]]),
                        "retire_compact_build_us": spread([x[3] for x in res["retire"]]),
                        "retire_wall_ms": spread([x[0] for x in res["retire"]]),
                        "retire_with_placement_rows_wall_ms": spread([x[0] for x in res["placed"]]),
                        "fork_device_us": spread([x[1] for x in res["fork"]]),
                        "fork_wall_ms": spread([x[0] for x in res["fork"]]),
                        "create_wall_ms": spread([x[0] for x in res["create"]])}}), flush=True)
                    del survivors, keep
                base.release()
                placed.release()
                del h_all, h_blob
    finally:
        eng.close()
        err.close()


if __name__ == "__main__":
    main()
