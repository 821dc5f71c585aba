#!/usr/bin/env python3
"""Node dict fold against the path it replaces, on one GPU listed W times: every
part holds a layer's result table and descriptors in HBM (n = 2k chunks per part,
every other one NEW) and the W x k NEW chunks are to join a node dict of m entries.

  fold       Node.dict_fold over the parts' device tables (ngpu_node_dict_fold)
  yardstick  what a caller did before: per part, copy both tables to the host,
             pick the NEW chunks out with numpy and build 80-B records; then one
             Node.dict_extend over the concatenated rows

Both run in place on a tip with room (each on its own fork of the base, made with
room for every round) and as a fork of the base, alternated, `rounds` times each
after one warm-up round.  Wall time is the whole path.  A node dict keeps
placements, so both paths carry k placement rows per part.  One GPU listed W
times says nothing about xGMI: every peer copy here stays inside one HBM.

usage: tools/node_dict_fold_bench.py [WS] [KS] [ROUNDS] [M]
       defaults: 2,8  128,16384  5  200000        -> JSON lines"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def main():
    import numpy as np
    import torch
    import nydus_gpu
    from nydus_gpu import rafs
    ws = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "2,8").split(",")]
    ks = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "128,16384").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    m = int(sys.argv[4]) if len(sys.argv) > 4 else 200000
    g = torch.Generator(device="cuda").manual_seed(0xF01D)
    rng = np.random.default_rng(0xF01D)
    modes = {"replicate": nydus_gpu.NODE_DICT_REPLICATE,
             "partition": nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY}

    def tables(k):
        """n = 2k chunks in HBM as a dedup call leaves them: even chunks NEW, odd INTRA."""
        n = 2 * k
        res = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
        res.random_(0, 256, generator=g)
        res[:, 32:40] = 0            # kind NEW, index 0
        res[1::2, 32] = 1            # INTRA
        ch = torch.zeros((n, 24), dtype=torch.uint8, device="cuda")
        ch[:, 10] = 0x10             # length 1 MiB
        return res, ch, n

    def step(W, k):
        t = [tables(k) for _ in range(W)]
        torch.cuda.synchronize()     # the fold reads the tables from its own streams
        parts = [{"d_results": r.data_ptr(), "d_chunks": c.data_ptr(), "n": n} for r, c, n in t]
        place = np.zeros(W * k, nydus_gpu.DICT_PLACE_DTYPE)
        place["compressed_size"] = 1 << 20
        return t, parts, place

    def rows_on_host(t, place):
        """The yardstick's host pass: every part's tables back, the NEW chunks as 80-B records."""
        out = []
        for res, ch, _ in t:
            r = res.cpu().numpy().view(nydus_gpu.RESULT_DTYPE).reshape(-1)
            c = ch.cpu().numpy().view(nydus_gpu.CHUNK_DTYPE).reshape(-1)
            new = r["kind"] == nydus_gpu.NEW
            rows = np.zeros(int(new.sum()), rafs.CHUNK_INFO_DTYPE)
            rows["block_id"] = r["digest"][new]
            rows["uncompressed_size"] = c["length"][new]
            rows["index"] = r["index"][new]
            rows["uncompressed_offset"] = r["uncompressed_offset"][new]
            out.append(rows)
        rows = np.concatenate(out)
        for f in ("compressed_offset", "compressed_size", "flags"):
            rows[f] = place[f]
        return rows

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, (time.perf_counter() - t0) * 1e3

    recs = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
    recs["block_id"] = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    recs["uncompressed_size"] = 1 << 20
    recs["compressed_size"] = 1 << 20
    for W in ws:
        node = nydus_gpu.Node([0] * W, digester="sha256")
        try:
            for mode, flag in modes.items():
                base = node.dict_create(recs, mode=flag)
                for k in ks:
                    # two tips with room for every round, one per path (a storage has one newest handle)
                    t, parts, place = step(W, (rounds + 2) * k + 1)
                    tip_f = node.dict_fold(base, parts, placements=place)
                    tip_y = node.dict_extend(base, rows_on_host(t, place))
                    del t, parts
                    torch.cuda.empty_cache()
                    assert not tip_f.info()["shares_base_storage"] and not tip_y.info()["shares_base_storage"]
                    res = {"fold_inplace": [], "yard_inplace": [], "fold_fork": [], "yard_fork": []}
                    for r in range(-1, rounds):  # round -1 warms every path up and is not kept
                        t, parts, place = step(W, k)
                        nxt, wall = timed(lambda: node.dict_fold(tip_f, parts, placements=place))
                        assert nxt.info()["shares_base_storage"] and nxt.entries == tip_f.entries + W * k, nxt.info()
                        tip_f.release()
                        tip_f = nxt
                        res["fold_inplace"].append(wall)
                        nxt, wall = timed(lambda: node.dict_extend(tip_y, rows_on_host(t, place)))
                        assert nxt.info()["shares_base_storage"] and nxt.entries == tip_y.entries + W * k, nxt.info()
                        tip_y.release()
                        tip_y = nxt
                        res["yard_inplace"].append(wall)
                        f, wall = timed(lambda: node.dict_fold(base, parts, placements=place))
                        assert not f.info()["shares_base_storage"] and f.entries == m + W * k
                        f.release()
                        res["fold_fork"].append(wall)
                        f, wall = timed(lambda: node.dict_extend(base, rows_on_host(t, place)))
                        assert not f.info()["shares_base_storage"] and f.entries == m + W * k
                        f.release()
                        res["yard_fork"].append(wall)
                        if r < 0:
                            for v in res.values():
                                v.clear()
                            continue
                        print(json.dumps({"W": W, "mode": mode, "dict_entries": m, "k_per_part": k, "n_per_part": 2 * k,
                                          "round": r, **{f"{op}_wall_ms": round(v[-1], 3) for op, v in res.items()}}),
                              flush=True)
                    s = {f"{op}_wall_ms": spread(v) for op, v in res.items()}
                    y = s["yard_inplace_wall_ms"]
                    # acceptance: in place, the fold is no slower than the yardstick beyond the yardstick's own spread
                    ok = s["fold_inplace_wall_ms"]["median"] <= y["median"] + (y["max"] - y["min"])
                    print(json.dumps({"W": W, "mode": mode, "dict_entries": m, "k_per_part": k, "n_per_part": 2 * k,
                                      "summary": s, "inplace_within_yardstick_spread": ok, "tip": tip_f.info()}),
                          flush=True)
                    tip_f.release()
                    tip_y.release()
                base.release()
        finally:
            node.close()


if __name__ == "__main__":
    main()
