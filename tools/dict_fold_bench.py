#!/usr/bin/env python3
"""Dict fold against the path it replaces, by dict size: a layer's result table
and descriptors lie in HBM (n = 2k chunks, every other one NEW) and its k NEW
chunks are to join a dict of m entries.

  fold       ChunkDict.fold over the device tables (ngpu_dict_fold)
  yardstick  what a caller did before: copy both tables to the host, pick the NEW
             chunks out with numpy, build 80-B records, ChunkDict.extend

Both run in place on a tip with room (each on its own fork of the base, made
with room for every round) and as a fork of the base, alternated, `rounds` times
each after one warm-up round.  Wall time is the whole path; device time comes from the library's
NGPU_DICT_TRACE lines (HIP events on its stream: a fold's keep + scan launches
plus its scatter + insert launches, an extend's unpack + insert launches; a fork
from before the device-to-device copy to the end of the table build).

usage: tools/dict_fold_bench.py [SIZES_M] [KS] [ROUNDS]
       defaults: 1,16,200  128,16384,1048576  5        -> JSON lines"""
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
os.environ["NGPU_DICT_TRACE"] = "1"  # read when the library first extends a dict


class Stderr:
    """fd 2 into a file while the library writes its trace lines there."""

    def __init__(self):
        self.saved = os.dup(2)
        self.tmp = tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 2)
        self.pos = 0

    def take(self):
        self.tmp.seek(self.pos)
        text = self.tmp.read().decode(errors="replace")
        self.pos += len(text.encode())
        return text

    def close(self):
        rest = self.take()
        os.dup2(self.saved, 2)
        if rest.strip():
            sys.stderr.write(rest)


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import rafs
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,16,200").split(",")]
    ks = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "128,16384,1048576").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    err = Stderr()
    eng = nydus_gpu.Engine(device=0, digester="sha256")
    g = torch.Generator(device="cuda").manual_seed(0xF01D)

    def tables(k):
        """n = 2k chunks in HBM as a dedup call leaves them: even chunks NEW, odd INTRA."""
        n = 2 * k
        res = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
        res.random_(0, 256, generator=g)
        res[:, 32:40] = 0            # kind NEW, index 0
        res[1::2, 32] = 1            # INTRA
        ch = torch.zeros((n, 24), dtype=torch.uint8, device="cuda")
        ch[:, 10] = 0x10             # length 1 MiB
        torch.cuda.synchronize()     # the fold reads the tables from its own stream
        return res, ch, n

    def rows_on_host(res, ch):
        """The yardstick's host pass: both tables back, the NEW chunks as 80-B records."""
        r = res.cpu().numpy().view(nydus_gpu.RESULT_DTYPE).reshape(-1)
        c = ch.cpu().numpy().view(nydus_gpu.CHUNK_DTYPE).reshape(-1)
        new = r["kind"] == nydus_gpu.NEW
        rows = np.zeros(int(new.sum()), rafs.CHUNK_INFO_DTYPE)
        rows["block_id"] = r["digest"][new]
        rows["uncompressed_size"] = c["length"][new]
        rows["index"] = r["index"][new]
        rows["uncompressed_offset"] = r["uncompressed_offset"][new]
        rows["compressed_size"] = rows["uncompressed_size"]
        return rows

    def timed(fn):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        text = err.take()
        f = re.findall(r"ngpu dict_fold (\w+) m=\d+ k=\d+ n=\d+ device_us=([0-9.]+) keep_scan_us=([0-9.]+)", text)
        x = re.findall(r"ngpu dict_extend (\w+) m=\d+ k=\d+ device_us=([0-9.]+)", text)
        if f:
            return out, wall, f[-1][0], float(f[-1][1]), float(f[-1][2])
        return out, wall, (x[-1][0] if x else None), (float(x[-1][1]) if x else None), None

    try:
        for mm in sizes:
            m = mm * 1_000_000
            dd = torch.empty((m, 32), dtype=torch.uint8, device="cuda")
            dd.random_(0, 256, generator=g)
            us = torch.full((m,), 1 << 20, dtype=torch.int32, device="cuda")
            bl = torch.zeros(m, dtype=torch.int32, device="cuda")
            ix = torch.arange(m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            base = eng.dict_create_device(dd.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), m, 1)
            del dd, us, bl, ix
            torch.cuda.empty_cache()
            for k in ks:
                # two tips with room for every round, one per path (a storage has one newest handle)
                seed = tables((rounds + 1) * k + 1)
                tip_f = base.fold(seed[0].data_ptr(), seed[1].data_ptr(), seed[2])
                tip_y = base.extend(rows_on_host(seed[0], seed[1]))
                del seed
                torch.cuda.empty_cache()
                assert not tip_f.info()["shares_base_storage"] and not tip_y.info()["shares_base_storage"]
                res = {"fold_inplace": [], "yard_inplace": [], "fold_fork": [], "yard_fork": []}
                for r in range(-1, rounds):  # round -1 warms every path up and is not kept
                    t_res, t_ch, n = tables(k)
                    nxt, wall, kind, dev, ks_us = timed(lambda: tip_f.fold(t_res.data_ptr(), t_ch.data_ptr(), n))
                    assert kind == "share" and nxt.entries == tip_f.entries + k, (kind, nxt.info())
                    tip_f.release()
                    tip_f = nxt
                    res["fold_inplace"].append((wall, dev, ks_us))
                    nxt, wall, kind, dev, _ = timed(lambda: tip_y.extend(rows_on_host(t_res, t_ch)))
                    assert kind == "share" and nxt.entries == tip_y.entries + k, (kind, nxt.info())
                    tip_y.release()
                    tip_y = nxt
                    res["yard_inplace"].append((wall, dev, None))
                    f, wall, kind, dev, ks_us = timed(lambda: base.fold(t_res.data_ptr(), t_ch.data_ptr(), n))
                    assert kind == "fork" and f.entries == m + k
                    f.release()
                    res["fold_fork"].append((wall, dev, ks_us))
                    f, wall, kind, dev, _ = timed(lambda: base.extend(rows_on_host(t_res, t_ch)))
                    assert kind == "fork" and f.entries == m + k
                    f.release()
                    res["yard_fork"].append((wall, dev, None))
                    if r < 0:
                        for v in res.values():
                            v.clear()
                        continue
                    print(json.dumps({"dict_entries": m, "k": k, "n": n, "round": r,
                                      **{f"{op}_wall_ms": round(v[-1][0], 3) for op, v in res.items()},
                                      **{f"{op}_device_us": v[-1][1] for op, v in res.items()},
                                      **{f"{op}_keep_scan_us": v[-1][2] for op, v in res.items()
                                         if v[-1][2] is not None}}), flush=True)
                print(json.dumps({"dict_entries": m, "k": k, "n": 2 * k, "summary": {
                    **{f"{op}_wall_ms": spread([x[0] for x in v]) for op, v in res.items()},
                    **{f"{op}_device_us": spread([x[1] for x in v]) for op, v in res.items()},
                    **{f"{op}_keep_scan_us": spread([x[2] for x in v]) for op, v in res.items()
                       if v[0][2] is not None}}, "tip": tip_f.info()}), flush=True)
                tip_f.release()
                tip_y.release()
            base.release()
    finally:
        eng.close()
        err.close()


if __name__ == "__main__":
    main()
