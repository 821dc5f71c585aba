#!/usr/bin/env python3
"""Dict save by dict size: what does writing a dict handle out as a RAFS v6 dict
bootstrap cost (ngpu_dict_save: records made on the GPU a window at a time, two
pinned windows on the host), next to the only way there was before it
(ngpu_dict_export into 80 x m bytes of host memory, rows converted on one host
thread, then one write of the same bytes)?

For each m a dict of m random rows in 10 blobs is made twice: from 80-B records in
host memory (it keeps placement rows, so every window uploads 16 B per row) and
from device arrays (no placement rows).  Then, alternated, `rounds` times each:
  (a) save to a writer that discards: the pipeline alone
  (b) save to a file (ngpu_write_fd)
  (c) export into host memory, then header + blob rows + records in one file
  (d) ngpu_dict_open of the file (b) wrote, for scale
and, for a partitioned node dict of the same rows on nodes [0] * W (one GPU listed W
times: the peer copies stay inside one HBM), Node.dict_save to a discarding writer
against Node.dict_export_parts.  The kernel's time per call next to the D2H time
comes from the library's NGPU_DICT_TRACE line (HIP events around every window's
kernel and copy).

usage: tools/dict_save_bench.py [LOG2_SIZES] [ROUNDS] [NODE_LOG2_SIZES] [NODE_W] [DIR]
       defaults: 20,24,26  5  20,24  2,8  the system's temporary directory  -> JSON lines
       (a size may also be given in rows, e.g. 200000000)"""
import ctypes
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first saves a dict

from dict_extend_bench import Stderr, spread  # noqa: E402

NB = 10
CS = 1 << 20
TRACE = (r"ngpu dict_save k=(\d+) parts=(\d+) place=(\d) windows=(\d+) window_records=(\d+) "
         r"kernel_us=([0-9.]+) d2h_us=([0-9.]+) kernel_us_max=([0-9.]+) d2h_us_max=([0-9.]+)")


def rows_of(x):
    v = int(x)
    return 1 << v if v < 64 else v


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import _lib, rafs
    arg = sys.argv[1:]
    sizes = [rows_of(x) for x in (arg[0] if len(arg) > 0 else "20,24,26").split(",") if x]
    rounds = int(arg[1]) if len(arg) > 1 else 5
    node_sizes = [rows_of(x) for x in (arg[2] if len(arg) > 2 else "20,24").split(",") if x]
    node_w = [int(x) for x in (arg[3] if len(arg) > 3 else "2,8").split(",") if x]
    tmp = arg[4] if len(arg) > 4 else tempfile.gettempdir()
    err = Stderr()
    L = nydus_gpu.lib()
    discard = _lib.WRITE_FN(lambda _c, _b, _n: 0)
    g = torch.Generator(device="cuda").manual_seed(0xD1C7)
    tbl = rafs.make_blob_table([f"{i:064x}" for i in range(NB)], CS, digester="sha256")

    def timed(fn):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        got = re.findall(TRACE, err.take())
        return out, wall, got[-1] if got else None

    def make_rows(m):
        d_recs = torch.empty((m, 80), dtype=torch.uint8, device="cuda")
        d_recs.random_(0, 256, generator=g)
        bl = (torch.arange(m, dtype=torch.int64, device="cuda") * NB // m).to(torch.int32)
        d_recs[:, 32:36] = bl.view(torch.uint8).reshape(m, 4)
        d_recs[:, 36:40] = 0     # flags
        d_recs[:, 64:72] = 0     # file_offset
        d_recs[:, 76:80] = 0     # reserved
        h = np.zeros((m, 80), np.uint8)
        torch.from_numpy(h).copy_(d_recs)
        return d_recs, bl, h

    def save_discard(call):
        info = _lib.NgpuDictSaveInfo()
        rc = call(None, discard, None, ctypes.byref(info))
        assert rc == 0, rc
        return info

    def trace_fields(t):
        return {"windows": int(t[3]), "window_records": int(t[4]), "kernel_us": float(t[5]), "d2h_us": float(t[6]),
                "kernel_us_max_window": float(t[7]), "d2h_us_max_window": float(t[8])}

    eng = nydus_gpu.Engine(device=0, digester="sha256", chunk_size=CS)
    try:
        for m in sizes:
            d_recs, bl, h_all = make_rows(m)
            path_b, path_c = os.path.join(tmp, f"dict_save_b_{m}.boot"), os.path.join(tmp, f"dict_save_c_{m}.boot")
            for placed in (True, False):
                if placed:
                    d = eng.dict_create(h_all, tbl)
                else:
                    dd = d_recs[:, :32].contiguous()
                    us = d_recs[:, 44:48].contiguous().view(torch.int32).reshape(m)
                    ix = d_recs[:, 72:76].contiguous().view(torch.int32).reshape(m)
                    uo = d_recs[:, 56:64].contiguous().view(torch.int64).reshape(m)
                    torch.cuda.synchronize()
                    d = eng.dict_create_device(dd.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), m, NB,
                                               d_uoff=uo.data_ptr())
                    del dd, us, ix, uo
                flag = 0 if placed else nydus_gpu.DICT_SAVE_NO_BLOB_TABLE
                opt = _lib.NgpuDictSaveOptions(flags=flag)
                res = {"a": [], "b": [], "c": [], "d": [], "k": [], "c2h": []}
                for r in range(rounds):
                    info, wall, t = timed(lambda: save_discard(
                        lambda _o, w, c, i: L.ngpu_dict_save(eng._h, d._h, ctypes.byref(opt), w, c, i)))
                    assert info.entries == m
                    tf = trace_fields(t)
                    res["a"].append(wall), res["k"].append(tf["kernel_us"]), res["c2h"].append(tf["d2h_us"])
                    _, wall_b, _ = timed(lambda: d.save(path_b, no_blob_table=not placed))
                    res["b"].append(wall_b)

                    def old_way():
                        recs, table = d.export()
                        head = rafs.write_v6_bootstrap(recs[:0], CS, flags=0x8,
                                                       blobs=None if table is None else np.frombuffer(table, rafs.BLOB_DTYPE))
                        head = bytearray(head)
                        head[rafs.EXT_OFFSET + 32:rafs.EXT_OFFSET + 40] = (80 * len(recs)).to_bytes(8, "little")
                        with open(path_c, "wb") as f:
                            f.write(head)
                            recs.tofile(f)
                    _, wall_c, _ = timed(old_way)
                    res["c"].append(wall_c)
                    row = {"dict_entries": m, "placement_rows": placed, "round": r, "file_bytes": int(info.bytes),
                           "save_discard_wall_ms": round(wall, 3), **tf, "save_file_wall_ms": round(wall_b, 3),
                           "export_then_write_wall_ms": round(wall_c, 3)}
                    if placed:  # (a file without a blob table opens too, but counts its blobs from the records)
                        o, wall_d, _ = timed(lambda: eng.dict_open(path_b))
                        assert o.entries == m
                        o.release()  # (the next round's save rewrites the file, so its open loads again)
                        res["d"].append(wall_d)
                        row["open_wall_ms"] = round(wall_d, 3)
                    print(json.dumps(row), flush=True)
                with open(path_b, "rb") as fb, open(path_c, "rb") as fc:  # the two ways agree
                    while True:
                        x, y = fb.read(1 << 26), fc.read(1 << 26)
                        assert x == y
                        if not x:
                            break
                print(json.dumps({"dict_entries": m, "placement_rows": placed, "summary": {
                    "save_discard_wall_ms": spread(res["a"]), "save_file_wall_ms": spread(res["b"]),
                    "export_then_write_wall_ms": spread(res["c"]),
                    **({"open_wall_ms": spread(res["d"])} if res["d"] else {}),
                    "kernel_us": spread(res["k"]), "d2h_us": spread(res["c2h"])}}), flush=True)
                d.release()
                for p in (path_b, path_c):
                    if os.path.exists(p):
                        os.unlink(p)
            del d_recs, bl, h_all
            torch.cuda.empty_cache()
    finally:
        eng.close()
    try:
        for W in node_w:
            node = nydus_gpu.Node([0] * W, digester="sha256", chunk_size=CS)
            try:
                for m in node_sizes:
                    d_recs, bl, h_all = make_rows(m)
                    del d_recs, bl
                    torch.cuda.empty_cache()
                    d = node.dict_create(h_all, tbl, mode=nydus_gpu.NODE_DICT_PARTITION)
                    res = {"save": [], "export": [], "k": [], "c2h": []}
                    for r in range(rounds):
                        info, wall, t = timed(lambda: save_discard(
                            lambda o, w, c, i: L.ngpu_node_dict_save(node._h, d._h, o, w, c, i)))
                        assert info.entries == m
                        tf = trace_fields(t)
                        got, wall_e, _ = timed(lambda: node.dict_export_parts(d))
                        assert len(got[0]) == m
                        del got
                        res["save"].append(wall), res["export"].append(wall_e)
                        res["k"].append(tf["kernel_us"]), res["c2h"].append(tf["d2h_us"])
                        print(json.dumps({"node_parts": W, "dict_entries": m, "round": r,
                                          "node_save_discard_wall_ms": round(wall, 3), **tf,
                                          "node_export_wall_ms": round(wall_e, 3)}), flush=True)
                    print(json.dumps({"node_parts": W, "dict_entries": m, "summary": {
                        "node_save_discard_wall_ms": spread(res["save"]), "node_export_wall_ms": spread(res["export"]),
                        "kernel_us": spread(res["k"]), "d2h_us": spread(res["c2h"])}}), flush=True)
                    d.release()
                    del h_all
            finally:
                node.close()
    finally:
        err.close()


if __name__ == "__main__":
    main()
