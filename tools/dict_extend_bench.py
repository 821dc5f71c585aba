#!/usr/bin/env python3
"""Dict extend by dict size: what does folding k records into a dict of m
entries cost when it is appended in place, when it forks (a new storage, the
base's records copied, the table rebuilt), and when the dict is rebuilt from
all m + k records with ngpu_dict_create?  The claim to confirm is structural:
the in-place device time at fixed k does not grow with m.

For each m a base of m random sha256-sized digests is created from device
arrays; one extend of it (a fork) gives a tip with room.  Then, alternated,
`rounds` times each: an in-place extend of the tip by k fresh records (the tip
moves on), a fork of the base by k records, and ngpu_dict_create over the
m + k records in host memory.  Wall time is the call; device time comes from
the library's NGPU_DICT_TRACE line (HIP events on its build stream: around the
unpack and insert launches of an in-place extend, around the copy, unpack and
table build of a fork).

usage: tools/dict_extend_bench.py [SIZES_M] [KS] [ROUNDS] [CREATE_ROUNDS_AT_200M]
       defaults: 1,16,200  128,16384  5  3        -> JSON lines"""
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
    ks = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "128,16384").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    big_rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    err = Stderr()
    eng = nydus_gpu.Engine(device=0, digester="sha256")
    g = torch.Generator(device="cuda").manual_seed(0xD1C7)
    rng = np.random.default_rng(0xD1C7)
    kmax = max(ks)

    def fresh(k):
        r = np.zeros(k, rafs.CHUNK_INFO_DTYPE)
        r["block_id"] = rng.integers(0, 256, (k, 32), dtype=np.uint8)
        r["uncompressed_size"] = 1 << 20
        r["index"] = np.arange(k)
        return r

    def timed(fn):
        err.take()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        us = re.findall(r"ngpu dict_extend (\w+) m=\d+ k=\d+ device_us=([0-9.]+)", err.take())
        return out, wall, (us[-1][0], float(us[-1][1])) if us else (None, None)

    try:
        for mm in sizes:
            m = mm * 1_000_000
            # m + kmax records in host memory (what a rebuild re-uploads), made on the GPU
            d_recs = torch.empty((m, 80), dtype=torch.uint8, device="cuda")
            d_recs.random_(0, 256, generator=g)
            d_recs[:, 32:36] = 0  # blob_index 0
            h_all = np.zeros((m + kmax, 80), np.uint8)
            torch.from_numpy(h_all[:m]).copy_(d_recs)
            dd = d_recs[:, :32].contiguous()
            del d_recs
            us = torch.full((m,), 1 << 20, dtype=torch.int32, device="cuda")
            bl = torch.zeros(m, dtype=torch.int32, device="cuda")
            ix = torch.arange(m, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()  # the build reads the arrays from its own stream
            base = eng.dict_create_device(dd.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), m, 1)
            del dd, us, bl, ix
            torch.cuda.empty_cache()
            tip = base.extend(fresh(kmax))  # a fork: half as many slots again
            assert not tip.info()["shares_base_storage"]
            for k in ks:
                res = {"inplace": [], "fork": [], "create": []}
                n_create = big_rounds if mm >= 100 else rounds
                for r in range(rounds):
                    fresh_k = fresh(k)
                    nxt, wall, (kind, dev) = timed(lambda: tip.extend(fresh_k))
                    assert kind == "share" and nxt.info()["shares_base_storage"], (kind, nxt.info())
                    tip.release()
                    tip = nxt
                    res["inplace"].append((wall, dev))
                    fresh_k = fresh(k)
                    f, wall, (kind, dev) = timed(lambda: base.extend(fresh_k))
                    assert kind == "fork" and f.entries == m + k
                    f.release()
                    res["fork"].append((wall, dev))
                    if r < n_create:
                        h_all[m:m + k] = fresh(k).view(np.uint8).reshape(k, 80)
                        c, wall, _ = timed(lambda: eng.dict_create(h_all[:m + k]))
                        assert c.entries == m + k
                        c.release()
                        res["create"].append((wall, None))
                    print(json.dumps({"dict_entries": m, "k": k, "round": r,
                                      **{f"{op}_wall_ms": round(v[-1][0], 3) for op, v in res.items() if len(v) > r},
                                      **{f"{op}_device_us": v[-1][1] for op, v in res.items()
                                         if len(v) > r and v[-1][1] is not None}}), flush=True)
                print(json.dumps({"dict_entries": m, "k": k, "summary": {
                    "inplace_device_us": spread([d for _, d in res["inplace"]]),
                    "inplace_wall_ms": spread([w for w, _ in res["inplace"]]),
                    "fork_device_us": spread([d for _, d in res["fork"]]),
                    "fork_wall_ms": spread([w for w, _ in res["fork"]]),
                    "create_wall_ms": spread([w for w, _ in res["create"]])},
                    "tip": tip.info()}), flush=True)
            tip.release()
            base.release()
            del h_all
    finally:
        eng.close()
        err.close()


if __name__ == "__main__":
    main()
