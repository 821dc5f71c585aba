#!/usr/bin/env python3
"""A/B of the host pipelines between two builds of libnydusgpu.so.

  python tools/host_ab.py --parent /path/to/other/libnydusgpu.so [--reps 15]

Both libraries are loaded into ONE process (two instances of the nydus_gpu
package, the other build through NYDUS_GPU_LIB) and work on the same host
buffers, their calls alternated and the order swapped every repetition:
Engine.verity (with and without the tree coming back), Engine.verity_verify
and Engine.check (`none` / `zstd` streams) of 2 GiB in host memory.  Runs of
one build in separate processes differ by more than two builds in one process
do (profiles/r8/README.md).
One JSON object per measurement on stdout; "parent" is the --parent build,
"branch" the one in the tree."""
import argparse
import importlib
import io
import json
import os
import statistics
import sys
import time

import torch  # before the library: one HIP runtime per process
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nydus-snapshotter_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def load(lib):
    for m in [m for m in sys.modules if m == "nydus_gpu" or m.startswith("nydus_gpu.")]:
        del sys.modules[m]
    if lib:
        os.environ["NYDUS_GPU_LIB"] = lib
    else:
        os.environ.pop("NYDUS_GPU_LIB", None)
    mod = importlib.import_module("nydus_gpu")
    mod.lib()
    return mod


ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="the other build of libnydusgpu.so")
ap.add_argument("--reps", type=int, default=15)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("host_ab: no GPU (there is no CPU fallback)")
P = load(os.path.abspath(args.parent))
B = load(None)  # stays in sys.modules: check_bench's layout() uses it
assert P is not B and P._lib.LIB_PATH != B._lib.LIB_PATH, (P._lib.LIB_PATH, B._lib.LIB_PATH)
import check_bench  # noqa: E402

REPS = args.reps
GiB, MiB = 1 << 30, 1 << 20


def alternate(name, fp, fb):
    fp(); fb()  # warm-up of both
    t = {"parent": [], "branch": []}
    for i in range(REPS):
        for tag, f in ((("parent", fp), ("branch", fb)) if i % 2 == 0 else (("branch", fb), ("parent", fp))):
            t0 = time.perf_counter()
            f()
            t[tag].append(time.perf_counter() - t0)
    row = {"measure": name, "reps": REPS}
    for tag, ts in t.items():
        row[tag] = {"s": [round(x, 4) for x in ts], "median_s": round(statistics.median(ts), 4),
                    "min_s": round(min(ts), 4), "max_s": round(max(ts), 4)}
    row["branch_over_parent_median"] = round(row["branch"]["median_s"] / row["parent"]["median_s"], 4)
    print(json.dumps(row), flush=True)


data = np.random.default_rng(11).integers(0, 256, 2 * GiB, dtype=np.uint8)
with P.Engine() as ep, B.Engine() as eb:
    stored, info = ep.verity(data)
    stored_b, info_b = eb.verity(data)
    assert info["root"] == info_b["root"] and np.array_equal(stored, stored_b)
    root = info["root"]
    del stored_b
    alternate("verity_host_2GiB_no_tree", lambda: ep.verity(data, want_tree=False),
              lambda: eb.verity(data, want_tree=False))
    alternate("verity_host_2GiB_tree", lambda: ep.verity(data), lambda: eb.verity(data))

    def ver(e):
        rep = e.verity_verify(data, stored, root)
        assert rep["bad"] == 0
    alternate("verity_verify_host_2GiB", lambda: ver(ep), lambda: ver(eb))
del data, stored

n_files, fs, cs = 512, 4 * MiB, MiB
headers, stride, total, ch = check_bench.layout(n_files, fs, cs)
tar = np.random.default_rng(11).integers(0, 16, total, dtype=np.uint8)
tar[: n_files * stride].reshape(n_files, stride)[:, :512] = headers
tar[n_files * stride:] = 0
with P.Engine(digester="blake3", chunk_size=cs) as ep, B.Engine(digester="blake3", chunk_size=cs) as eb:
    for comp in ("none", "zstd"):
        w = eb.pack(retain=True)
        w.write(tar)
        o = io.BytesIO()
        w.finish(o, compressor=comp)
        stream = np.frombuffer(o.getbuffer(), np.uint8)

        def chk(e):
            rep = e.check(stream)
            assert rep["bad"] == 0 and rep["checked"] == len(ch), rep
        alternate("check_host_2GiB_" + comp, lambda: chk(ep), lambda: chk(eb))
        del stream, o
