#!/usr/bin/env python3
"""Check (ngpu_check_device / ngpu_check_stream) measurements for DESIGN §3.

  python tools/check_bench.py --device   # the verdict kernel's added time on a C2-shaped layer
  python tools/check_bench.py --host     # 2 GiB `none` / `zstd` streams against the CPU re-digest

--device: a 16 GiB layer (4096 x 4 MiB files, 1 MiB chunks) resident in HBM;
  `calls` back-to-back ngpu_digest_device calls between two HIP events, then as
  many ngpu_check_device calls (expected digests at stride 32), alternating
  for `rounds` rounds.  Reports the median per-call time of each and the
  difference: the verdict kernel + the counters' memset.
--host: a 2 GiB layer tar (512 x 4 MiB files of random nibbles, so zstd halves
  them) packed through the GPU writer with compressor none and zstd; the wall
  time of Engine.check(stream) from host memory (the call ends synchronised),
  against the same chunks re-digested on the CPU: the oracle's digest_chunks
  on 16 threads, and the project's CPU baseline (SIMD digests on 16 threads +
  stream dedup).  The CPU figures hash the chunks already
  inflated: no inflate is charged to them.
One JSON object per measurement on stdout."""
import argparse
import io
import json
import os
import statistics
import sys
import tarfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch  # before the library: one HIP runtime per process
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nydus-snapshotter_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nydus_gpu  # noqa: E402

MiB = 1 << 20


def layout(n_files, file_size, chunk):
    """Tar headers, per-file stride, total bytes and the chunk descriptors."""
    stride = 512 + file_size
    per = file_size // chunk
    ch = np.zeros(n_files * per, nydus_gpu.CHUNK_DTYPE)
    i = np.repeat(np.arange(n_files, dtype=np.uint64), per)
    k = np.tile(np.arange(per, dtype=np.uint64), n_files)
    ch["offset"] = i * np.uint64(stride) + np.uint64(512) + k * np.uint64(chunk)
    ch["length"] = chunk
    ch["file_index"] = i
    ch["file_offset"] = k * np.uint64(chunk)
    headers = np.zeros((n_files, 512), np.uint8)
    for f in range(n_files):
        ti = tarfile.TarInfo(f"usr/lib/file-{f:05d}.bin")
        ti.size, ti.mode, ti.mtime = file_size, 0o644, 0
        headers[f] = np.frombuffer(ti.tobuf(format=tarfile.GNU_FORMAT), np.uint8)
    return headers, stride, n_files * stride + 1024, ch


def device_stage(calls, rounds):
    n_files, fs, cs = 4096, 4 * MiB, MiB
    headers, stride, total, ch = layout(n_files, fs, cs)
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(7)
    for s in range(0, total, 1 << 30):
        buf[s:min(total, s + (1 << 30))].random_(0, 256, generator=g)
    buf[: n_files * stride].view(n_files, stride)[:, :512].copy_(torch.from_numpy(headers).cuda())
    n = len(ch)
    d_ch = torch.from_numpy(ch.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_bm = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    eng = nydus_gpu.Engine(digester="blake3", chunk_size=cs)
    try:
        def digest():
            eng.digest_device(buf.data_ptr(), total, d_ch.data_ptr(), n, d_out.data_ptr(), stream=s)

        def check():
            eng.check_device(buf.data_ptr(), total, d_ch.data_ptr(), n, d_out.data_ptr(), d_exp.data_ptr(), 32,
                             d_bm.data_ptr(), d_cnt.data_ptr(), stream=s)
        digest()
        torch.cuda.synchronize()
        d_exp = d_out.view(n, 64)[:, :32].contiguous()
        check()  # warm-up, and the verdict on clean input
        torch.cuda.synchronize()
        clean = (d_cnt.cpu().tolist(), int((d_bm != 0).sum()))
        d_exp[n - 1, 5] ^= 1
        check()
        torch.cuda.synchronize()
        one = (d_cnt.cpu().tolist(), d_bm[-1].item() & (2 ** 64 - 1), int((d_bm != 0).sum()))
        d_exp[n - 1, 5] ^= 1
        assert clean == ([0, 0], 0) and one == ([1, 0], 1 << ((n - 1) % 64), 1), (clean, one)
        t = {"digest": [], "check": []}
        for _ in range(rounds):
            for name, fn in (("digest", digest), ("check", check)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                torch.cuda.synchronize()
                t[name].append(a.elapsed_time(b) / calls)
        eng.device_status()
    finally:
        eng.close()
    md, mc = statistics.median(t["digest"]), statistics.median(t["check"])
    return {"measure": "device_stage", "layer_bytes": total, "chunks": n, "calls_per_window": calls,
            "digest_ms": [round(x, 4) for x in t["digest"]], "check_ms": [round(x, 4) for x in t["check"]],
            "digest_ms_median": round(md, 4), "check_ms_median": round(mc, 4),
            "added_ms": round(mc - md, 4), "added_pct": round(100 * (mc - md) / md, 2),
            "check_TBps": round(total / mc / 1e9, 3)}


def host_pipeline(reps):
    import oracle_py
    n_files, fs, cs = 512, 4 * MiB, MiB
    headers, stride, total, ch = layout(n_files, fs, cs)
    rng = np.random.default_rng(11)
    tar = rng.integers(0, 16, total, dtype=np.uint8)  # nibbles: zstd stores about half
    tar[: n_files * stride].reshape(n_files, stride)[:, :512] = headers
    tar[n_files * stride:] = 0
    assert np.array_equal(nydus_gpu.tar_chunks(tar, cs), ch)
    out = []
    # the CPU re-digest of the same chunks (already inflated)
    och = ch.view(oracle_py.CHUNK_DTYPE)
    t_cpu = []
    with ThreadPoolExecutor(16) as ex:
        for _ in range(reps):
            t0 = time.perf_counter()
            list(ex.map(lambda part: oracle_py.digest_chunks(tar, part, "blake3"), np.array_split(och, 16)))
            t_cpu.append(time.perf_counter() - t0)
    t_base = []
    for _ in range(reps):
        t0 = time.perf_counter()
        oracle_py.cpu_digest_dedup(tar, och, "blake3", 16)
        t_base.append(time.perf_counter() - t0)
    ubytes = int(ch["length"].sum())
    cpu = {"measure": "cpu_redigest", "bytes": ubytes, "impl": oracle_py.cpu_impl(),
           "digest_chunks_16_threads_s": [round(x, 4) for x in t_cpu],
           "digest_chunks_16_threads_GBps": round(ubytes / min(t_cpu) / 1e9, 2),
           "cpu_baseline_16_threads_s": [round(x, 4) for x in t_base],
           "cpu_baseline_16_threads_GBps": round(ubytes / min(t_base) / 1e9, 2)}
    out.append(cpu)
    with nydus_gpu.Engine(digester="blake3", chunk_size=cs) as eng:
        for comp in ("none", "zstd"):
            w = eng.pack(retain=True)
            w.write(tar)
            o = io.BytesIO()
            w.finish(o, compressor=comp)
            stream = np.frombuffer(o.getbuffer(), np.uint8)
            rep = eng.check(stream)  # warm-up: pins and allocates nothing that is kept, loads the codec
            assert rep["bad"] == 0 and rep["bytes"] == ubytes and rep["checked"] == len(ch), rep
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                rep = eng.check(stream)
                ts.append(time.perf_counter() - t0)
            assert rep["bad"] == 0
            out.append({"measure": "host_pipeline", "compressor": comp, "stream_bytes": int(stream.size),
                        "uncompressed_bytes": ubytes, "records": rep["records"],
                        "check_s": [round(x, 4) for x in ts],
                        "check_GBps_uncompressed": round(ubytes / min(ts) / 1e9, 2),
                        "vs_digest_chunks_16_threads": round(min(t_cpu) / min(ts), 2),
                        "vs_cpu_baseline_16_threads": round(min(t_base) / min(ts), 2)})
            del stream, o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("check_bench: no GPU (there is no CPU fallback)")
    if args.device or not args.host:
        print(json.dumps(device_stage(args.calls, args.rounds)), flush=True)
    if args.host or not args.device:
        for r in host_pipeline(args.reps):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
