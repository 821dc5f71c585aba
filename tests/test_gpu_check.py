"""GPU: Check -- re-digest a converted layer's chunks and compare them with the
digests its bootstrap records (ngpu_check_device / ngpu_check_image /
ngpu_check_stream, csrc/check.hip).

The reference proves a conversion by reading it back (`nydusify check`,
tests/converter_test.go:865-875; nydusd `digest_validate`, tests/nydusd.go:69).
Pinned here:
* the device stage: the verdict bitmap and counters for ragged chunks, both
  digesters, every n around the wave (64) and workgroup (256) edges, expected
  digests at stride 32, 80 (inside RAFS v6 chunk-info records) and 36 (dword
  loads), with the bitmap pre-filled with 0xFF and the counters with garbage;
* the stream form on clean streams of every compressor, both digesters, RAFS
  v5 and v6, CPU- and GPU-written;
* every failure reason (DIGEST by data and by block_id, DECOMPRESS, RANGE,
  DICT), windows, the failure cap, node dicts and the engine mismatches.
Expected digests come from the CPU oracle."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import blob_ref
import nydus_gpu
from nydus_gpu import rafs

from conftest import ROOT

pytestmark = pytest.mark.gpu

CS = 0x1000
NS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
GARBAGE = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- device stage -----------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(oracle):
    """1000 chunks of 1..4096 bytes at 512-aligned offsets (chunk size 0x1000),
    their oracle digests for both digesters, all uploaded once."""
    import b3_shapes
    rng = np.random.default_rng(0xC4EC)
    lens = [1, 4096, 4095, 1023, 1024, 1025, 64, 65] + [int(x) for x in rng.integers(1, 4097, 992)]
    offs, pos = [], 0
    for ln in lens:
        pos = (pos + 511) & ~511
        offs.append(pos)
        pos += ln
    data, ch = b3_shapes._finish(rng, [(ln, 0) for ln in lens], offs, pos, [])
    digs = {d: oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), d) for d in ("blake3", "sha256")}
    return {"len": len(data), "d_data": _dev(np.frombuffer(data, np.uint8)), "d_ch": _dev(ch),
            "digs": digs}


def _layout(dig, stride):
    """The expected digests at a byte stride, as a uint8 buffer."""
    n = len(dig)
    if stride == 32:
        return dig.copy().reshape(-1)
    if stride == 80:  # block_id of RAFS v6 chunk-info records, the other fields noise
        recs = np.frombuffer(np.full(n * 80, 0xEE, np.uint8).tobytes(), rafs.CHUNK_INFO_DTYPE).copy()
        recs["block_id"] = dig
        return recs.view(np.uint8).reshape(-1)
    buf = np.full(n * stride + 4, 0xEE, np.uint8)
    for i in range(n):
        buf[i * stride:i * stride + 32] = dig[i]
    return buf


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("digester", ["blake3", "sha256"])
def test_check_device_bitmap_and_counts(ragged, digester, n):
    dig = ragged["digs"][digester][:n]
    words = (n + 63) // 64
    sets = [set(), {0}, {n - 1}, {63, 64}, set(range(n))]
    sets = [s for i, s in enumerate(sets) if i == 0 or (s and min(s) >= 0 and max(s) < n)]
    eng = nydus_gpu.Engine(digester=digester, chunk_size=CS)
    try:
        for stride in (32, 80, 36):
            for flip in sets:
                exp = dig.copy()
                for i in flip:
                    exp[i, (7 * i + 3) % 32] ^= 1 << (i % 8)
                buf = _layout(exp, stride)
                d_exp = _dev(buf) if buf.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
                d_out = torch.zeros(max(n, 1) * 64, dtype=torch.uint8, device="cuda")
                # one guard word behind the bitmap: the call writes (n + 63) / 64 words, no more
                d_bm = torch.full((words + 1,), -1, dtype=torch.int64, device="cuda")
                d_cnt = torch.full((2,), GARBAGE, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                eng.check_device(ragged["d_data"].data_ptr(), ragged["len"], ragged["d_ch"].data_ptr(), n,
                                 d_out.data_ptr(), d_exp.data_ptr(), stride, d_bm.data_ptr(),
                                 d_cnt.data_ptr())
                torch.cuda.synchronize()
                bm = d_bm.cpu().numpy().view(np.uint64)
                cnt = d_cnt.cpu().numpy().view(np.uint64)
                got = set(np.flatnonzero(np.unpackbits(bm[:words].view(np.uint8), bitorder="little")).tolist())
                what = (digester, n, stride, sorted(flip)[:4])
                assert got == flip, what  # exactly the flipped records; zero words and tail bits written
                assert bm[words] == np.uint64(0xFFFFFFFFFFFFFFFF), what
                assert (int(cnt[0]), int(cnt[1])) == (len(flip), 0), what
                out = d_out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)[:n]
                assert np.array_equal(out["digest"], dig), what
                assert (out["kind"] == nydus_gpu.DIGESTED).all(), what
    finally:
        eng.close()


@pytest.mark.parametrize("digester", ["blake3", "sha256"])
def test_check_device_counts_records_the_digest_stage_rejected(ragged, digester):
    """The `kind != NGPU_DIGESTED` leg: descriptors past the data buffer are
    rejected by the digest stage (bounds-checked; ngpu_device_status reports
    them, tests/test_gpu_guard.py), so their records keep no digest.  They are
    bad whatever the expected bytes say, and counted in d_counts[1]."""
    n, out_of_range, flipped = 130, [5, 70], [64, 129]
    ch = ragged["d_ch"].cpu().numpy().view(nydus_gpu.CHUNK_DTYPE)[:n].copy()
    ch["offset"][out_of_range] = ragged["len"]  # past the buffer
    exp = ragged["digs"][digester][:n].copy()
    for i in flipped:
        exp[i, 0] ^= 1
    d_ch, d_exp = _dev(ch), _dev(exp)
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_bm = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((2,), GARBAGE, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with nydus_gpu.Engine(digester=digester, chunk_size=CS) as eng:
        eng.check_device(ragged["d_data"].data_ptr(), ragged["len"], d_ch.data_ptr(), n, d_out.data_ptr(),
                         d_exp.data_ptr(), 32, d_bm.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.device_status()
        assert e.value.code == nydus_gpu.EINVAL and "outside" in str(e.value)
        eng.device_status()  # cleared
    bm = d_bm.cpu().numpy().view(np.uint64)
    got = set(np.flatnonzero(np.unpackbits(bm[:3].view(np.uint8), bitorder="little")).tolist())
    assert got == set(out_of_range + flipped)
    assert bm[3] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert d_cnt.cpu().tolist() == [4, 2]
    out = d_out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
    assert (out["kind"][out_of_range] != nydus_gpu.DIGESTED).all()
    ok = np.setdiff1d(np.arange(n), out_of_range)
    assert np.array_equal(out["digest"][ok], ragged["digs"][digester][:n][ok])


def test_check_device_rejects_bad_stride_and_base(ragged):
    n = 64
    d_exp = _dev(np.zeros(n * 80 + 16, np.uint8))
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_bm = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    eng = nydus_gpu.Engine(chunk_size=CS)
    try:
        for base, stride in ((0, 30), (0, 28), (0, 34), (2, 32), (2, 80)):
            with pytest.raises(nydus_gpu.NgpuError) as e:
                eng.check_device(ragged["d_data"].data_ptr(), ragged["len"], ragged["d_ch"].data_ptr(), n,
                                 d_out.data_ptr(), d_exp.data_ptr() + base, stride, d_bm.data_ptr(),
                                 d_cnt.data_ptr())
            assert e.value.code == nydus_gpu.EINVAL, (base, stride)
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.check_device(ragged["d_data"].data_ptr(), ragged["len"], ragged["d_ch"].data_ptr(),
                             0xFFFFFFFF, d_out.data_ptr(), d_exp.data_ptr(), 32, d_bm.data_ptr(),
                             d_cnt.data_ptr())
        assert e.value.code == nydus_gpu.EINVAL
    finally:
        eng.close()
    torch.cuda.synchronize()


# ---- streams ------------------------------------------------------------------
S = 0x10000


@pytest.fixture(scope="module")
def streams(oracle, tars):
    """CPU-written streams, built once: (layer, compressor, digester) -> bytes."""
    from test_blob import cpu_stream
    cache = {}

    def get(name, compressor, digester="blake3", tar=None):
        key = (name, compressor, digester)
        if key not in cache:
            cache[key] = cpu_stream(oracle, tars[name] if tar is None else tar, S, compressor, digester)[0]
        return cache[key]
    return get


def _records(stream):
    """image.boot of a v6 stream: (its offset in the stream, read_v6 dict)."""
    off, size = blob_ref.seek_file_by_tar_header(stream, "image.boot")
    v6 = rafs.read_v6(stream[off:off + size])
    return off, v6


def _patch(stream, j, field, fn):
    """The stream with `field` of chunk record j of its image.boot changed by fn."""
    off, v6 = _records(stream)
    dt = rafs.CHUNK_INFO_DTYPE
    fdt, foff = dt.fields[field][0], dt.fields[field][1]
    at = off + v6["chunk_table_offset"] + 80 * j + foff
    out = bytearray(stream)
    old = np.frombuffer(bytes(out[at:at + fdt.itemsize]), fdt.base)
    new = np.asarray(fn(old if fdt.shape else old[0])).astype(fdt.base).tobytes()
    assert len(new) == fdt.itemsize
    out[at:at + fdt.itemsize] = new
    return bytes(out)


def _flip_data(stream, recs, k):
    """The stream with one byte inside record k's compressed range flipped."""
    out = bytearray(stream)
    at = int(recs[k]["compressed_offset"]) + int(recs[k]["compressed_size"]) // 2
    out[at] ^= 0x40
    return bytes(out)


def _ids(rep):
    return [(b["blob_index"], b["index"], b["reason"]) for b in rep["bad_list"]]


def _rid(rec, reason):
    return (int(rec["blob_index"]), int(rec["index"]), reason)


def _assert_clean(rep, recs):
    assert rep["bad"] == 0 and rep["bad_list"] == [], rep
    assert rep["checked"] == rep["records"] == len(recs), rep
    assert rep["bytes"] == int(recs["uncompressed_size"].sum()), rep
    assert rep["skipped"] == rep["dict_checked"] == rep["dict_bad"] == 0, rep


@pytest.mark.parametrize("name", ["oci_lower", "edge_pax"])
@pytest.mark.parametrize("digester", ["blake3", "sha256"])
@pytest.mark.parametrize("compressor", ["none", "zstd", "lz4_block"])
def test_check_clean_stream(streams, compressor, digester, name):
    stream = streams(name, compressor, digester)
    recs = _records(stream)[1]["chunks"]
    assert len(recs) > 0
    if compressor != "none" and name == "edge_pax":
        assert (recs["flags"] & 1).any()  # some chunk really is inflated
    with nydus_gpu.Engine(digester=digester, chunk_size=S) as eng:
        _assert_clean(eng.check(stream), recs)


def test_check_clean_v5_and_gpu_written_streams(tars):
    for fsv in (5, 6):
        with nydus_gpu.Engine(chunk_size=S, fs_version=fsv) as eng:
            w = eng.pack(retain=True)
            w.write(tars["edge_pax"])
            o = io.BytesIO()
            w.finish(o, compressor="zstd")
            stream = o.getvalue()
            rep = eng.check(stream)
            boot = blob_ref.unpack_entry(stream, "image.boot")[0]
            assert rafs.detect_fs_version(boot) == f"v{fsv}"
            dump = nydus_gpu.rafs_dump(boot)
            distinct = {(c[1], c[8]): c[6] for i in dump["inodes"] for c in i.get("chunks", [])}
            assert rep["bad"] == 0 and rep["bad_list"] == [], (fsv, rep)
            assert rep["checked"] == rep["records"] == len(distinct) > 0, (fsv, rep)
            assert rep["bytes"] == sum(distinct.values()) and rep["skipped"] == 0, (fsv, rep)


@pytest.mark.parametrize("digester", ["blake3", "sha256"])
def test_check_finds_corrupted_data(oracle, streams, digester):
    stream = streams("edge_pax", "none", digester)
    recs = _records(stream)[1]["chunks"]
    with nydus_gpu.Engine(digester=digester, chunk_size=S) as eng:
        for k in (0, len(recs) - 1, len(recs) // 2):
            bad = _flip_data(stream, recs, k)
            rep = eng.check(bad)
            assert rep["bad"] == 1 and _ids(rep) == [_rid(recs[k], "DIGEST")], (k, rep)
            assert rep["checked"] == rep["records"] == len(recs)
            b = rep["bad_list"][0]
            a, n = int(recs[k]["compressed_offset"]), int(recs[k]["compressed_size"])
            assert b["expected"] == bytes(recs[k]["block_id"]).hex()
            assert b["got"] == oracle.digest(bad[a:a + n], digester).hex()
            assert b["uncompressed_size"] == n and b["compressed_offset"] == a


@pytest.mark.parametrize("compressor", ["none", "zstd", "lz4_block"])
def test_check_finds_corrupted_block_id(oracle, streams, compressor):
    stream = streams("edge_pax", compressor)
    off, v6 = _records(stream)
    recs = v6["chunks"]
    assert stream[off:off + 8] == blob_ref.unpack_entry(stream, "image.boot")[0][:8]
    with nydus_gpu.Engine(chunk_size=S) as eng:
        for j in (0, len(recs) - 1, 3):
            bad = _patch(stream, j, "block_id", lambda d: d ^ np.eye(1, 32, 9, dtype=np.uint8)[0] * 4)
            rep = eng.check(bad)
            assert rep["bad"] == 1 and _ids(rep) == [_rid(recs[j], "DIGEST")], (j, rep)
            b = rep["bad_list"][0]
            want = bytearray(bytes(recs[j]["block_id"]))
            want[9] ^= 4
            assert b["expected"] == bytes(want).hex()
            assert b["got"] == bytes(recs[j]["block_id"]).hex()  # the bytes still hash to the true digest


def test_check_lists_truncated_frame_and_range_and_goes_on(streams):
    stream = streams("edge_pax", "zstd")
    recs = _records(stream)[1]["chunks"]
    j = int(np.flatnonzero(recs["flags"] & 1)[0])
    r = (j + 2) % len(recs)
    bad = _patch(stream, j, "compressed_size", lambda v: v - 3)  # the zstd frame loses its end
    bad = _patch(bad, r, "compressed_offset", lambda v: len(stream) + 1)  # past the stream
    with nydus_gpu.Engine(chunk_size=S) as eng:
        rep = eng.check(bad)
    want = sorted([(j, "DECOMPRESS"), (r, "RANGE")])
    assert rep["bad"] == 2 and _ids(rep) == [_rid(recs[i], why) for i, why in want], rep
    assert all(b["got"] == "00" * 32 for b in rep["bad_list"])
    # the remaining records were still checked on the GPU
    assert rep["checked"] == rep["records"] == len(recs)
    assert rep["bytes"] == int(recs["uncompressed_size"].sum()) - sum(int(recs[i]["uncompressed_size"])
                                                                      for i in (j, r))


def test_check_image_takes_blob_data_or_whole_streams(streams):
    stream = streams("edge_pax", "zstd")
    v6 = _records(stream)[1]
    recs, bid = v6["chunks"], v6["blob_ids"][0]
    boot = blob_ref.unpack_entry(stream, "image.boot")[0]
    blob = blob_ref.unpack_entry(stream, "image.blob")[0]
    assert stream[:len(blob)] == blob  # compressed_offset counts from offset 0 in both
    k = int(np.flatnonzero((recs["flags"] & 1) == 0)[1])  # a chunk stored raw
    bad = bytearray(blob)
    bad[int(recs[k]["compressed_offset"])] ^= 0x80
    with nydus_gpu.Engine(chunk_size=S) as eng:
        for data in (blob, stream):
            _assert_clean(eng.check_image(boot, {bid: data}), recs)
        rep = eng.check_image(boot, {bid: bytes(bad)})
        assert rep["bad"] == 1 and _ids(rep) == [_rid(recs[k], "DIGEST")], rep
        for blobs in ({}, {"00" * 32: blob}):  # the record's blob is not among them
            rep = eng.check_image(boot, blobs)
            assert (rep["records"], rep["checked"], rep["skipped"], rep["bad"]) == (len(recs), 0, len(recs), 0)
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.check_image(boot[:2000], {bid: blob})
        assert e.value.code == nydus_gpu.EFORMAT


# ---- windows, caps ------------------------------------------------------------
def _plan(sizes, window):
    """csrc/check_plan.hpp restated: the window each record lands in."""
    win, at, out = 0, 0, []
    for i, s in enumerate(sizes):
        a = (at + 15) // 16 * 16
        if i and a + s > window:
            win, a = win + 1, 0
        out.append(win)
        at = a + s
    return out


def test_check_windows_give_the_one_window_report(streams):
    import layers
    window = 1 << 20
    t = layers._TarBuilder()  # ~5 MB of distinct chunks, then a small file
    t.file("big", layers.prng_bytes(0xC4EC, 5 * (1 << 20) + 333))
    t.file("small", b"tail")
    stream = streams("five_mb", "none", tar=t.bytes())
    recs = _records(stream)[1]["chunks"]
    wins = _plan([int(x) for x in recs["uncompressed_size"]], window)
    assert wins[-1] + 1 >= 4 and int(recs["uncompressed_size"].sum()) > 4 * window
    first = wins.index(2)                      # the first record of a window
    last = wins.index(2) - 1                   # the last record of the window before it
    tail = len(recs) - 1                       # in the last window
    assert wins[last] == 1 and wins[tail] == wins[-1]
    with nydus_gpu.Engine(chunk_size=S) as eng:
        def windows(**kw):  # the report, and how many windows went to the GPU for it
            before = eng.counters()["check_windows"]
            rep = eng.check(**kw)
            return rep, eng.counters()["check_windows"] - before
        rep, nw = windows(stream=stream, window_bytes=window)
        _assert_clean(rep, recs)
        assert nw == wins[-1] + 1 >= 4
        for ks in ([first], [last], [tail], [last, first, tail]):
            bad = stream
            for k in ks:
                bad = _flip_data(bad, recs, k)
            one, nw1 = windows(stream=bad)
            many, nwm = windows(stream=bad, window_bytes=window)
            assert (nw1, nwm) == (1, wins[-1] + 1), ks
            assert many == one, ks
            assert one["bad"] == len(ks) and _ids(one) == [_rid(recs[k], "DIGEST") for k in sorted(ks)], ks
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.check(stream, window_bytes=S - 16)
        assert e.value.code == nydus_gpu.EINVAL


def test_check_cap_keeps_record_order_across_failure_kinds(streams):
    """An inflate failure (found while a window is filled) at an earlier record
    than a RANGE failure (found before any window runs), and a DIGEST failure
    before both: every cap lists a prefix of the record order."""
    stream = streams("edge_pax", "zstd")
    recs = _records(stream)[1]["chunks"]
    j = int(np.flatnonzero(recs["flags"] & 1)[0])
    g, r = j - 1, len(recs) - 1
    assert 0 <= g and not recs[g]["flags"] & 1 and j < r
    bad = _flip_data(stream, recs, g)                                      # DIGEST at g
    bad = _patch(bad, j, "compressed_size", lambda v: v - 3)               # DECOMPRESS at j > g
    bad = _patch(bad, r, "compressed_offset", lambda v: len(stream) + 1)   # RANGE at r > j
    want = [_rid(recs[g], "DIGEST"), _rid(recs[j], "DECOMPRESS"), _rid(recs[r], "RANGE")]
    with nydus_gpu.Engine(chunk_size=S) as eng:
        for cap in (1, 2, 3, 64):
            rep = eng.check(bad, max_bad=cap)
            assert rep["bad"] == 3 and _ids(rep) == want[:cap], (cap, rep)
        # and with the DECOMPRESS failure first
        bad2 = _patch(_patch(stream, j, "compressed_size", lambda v: v - 3), r, "compressed_offset",
                      lambda v: len(stream) + 1)
        rep = eng.check(bad2, max_bad=1)
        assert rep["bad"] == 2 and _ids(rep) == [_rid(recs[j], "DECOMPRESS")], rep


def test_check_caps_the_list_not_the_count(streams):
    stream = streams("edge_pax", "none")
    recs = _records(stream)[1]["chunks"]
    assert len(recs) >= 11
    ks = [9, 1, 6, 4, len(recs) - 1]
    bad = stream
    for k in ks:
        bad = _flip_data(bad, recs, k)
    with nydus_gpu.Engine(chunk_size=S) as eng:
        rep = eng.check(bad, max_bad=2)
        assert rep["bad"] == 5 and _ids(rep) == [_rid(recs[k], "DIGEST") for k in (1, 4)], rep
        rep = eng.check(bad, max_bad=0)
        assert rep["bad"] == 5 and rep["bad_list"] == []


# ---- dict references ------------------------------------------------------------
DICT_ID = "ab" * 32


@pytest.fixture(scope="module")
def dict_case(oracle, tars, tmp_path_factory):
    """oci_lower / oci_upper packed against the chunk_dict bootstrap, as
    test_node_packs_round_robin_write_dict_records does."""
    from test_blob import cpu_stream
    cs = 0x100000
    with nydus_gpu.Engine(chunk_size=cs) as eng:
        ch, out, _ = eng.pack_tar(tars["chunk_dict"])
        tab = nydus_gpu.chunk_table(ch, out).view(rafs.CHUNK_INFO_DTYPE).reshape(-1)
    blobs = rafs.make_blob_table([DICT_ID], cs, counts=[len(tab)])
    boot = rafs.write_v6_bootstrap(tab, cs, flags=0x5, blobs=blobs)
    path = tmp_path_factory.mktemp("check") / "dict-bootstrap"
    path.write_bytes(boot)
    out = {"cs": cs, "tab": tab, "blobs": blobs, "path": str(path), "dir": path.parent}
    for name in ("oci_lower", "oci_upper"):
        out[name] = cpu_stream(oracle, tars[name], cs, "none", dict_boot=boot)[0]
    return out


def _dict_records(stream):
    v6 = _records(stream)[1]
    recs = v6["chunks"]
    return recs, np.array([v6["blob_ids"][int(b)] == DICT_ID for b in recs["blob_index"]], bool)


def test_check_resolves_dict_records(dict_case):
    total = 0
    with nydus_gpu.Engine(chunk_size=dict_case["cs"]) as eng:
        d = eng.dict_open(dict_case["path"])
        for name in ("oci_upper", "oci_lower"):
            stream = dict_case[name]
            recs, isdict = _dict_records(stream)
            nd = int(isdict.sum())
            total += nd
            rep = eng.check(stream, dict=d)
            assert rep["records"] == len(recs) and rep["checked"] == len(recs) - nd, (name, rep)
            assert (rep["dict_checked"], rep["dict_bad"], rep["skipped"], rep["bad"]) == (nd, 0, 0, 0), (name, rep)
            rep = eng.check(stream)  # no dict: the same records are skipped
            assert (rep["dict_checked"], rep["skipped"], rep["bad"]) == (0, nd, 0), (name, rep)
            assert rep["checked"] == len(recs) - nd
        d.release()
    assert total > 0  # oci_lower shares its dir-1 files with the chunk dict


def test_check_lists_a_record_the_dict_places_elsewhere(dict_case):
    stream = dict_case["oci_lower"]
    recs, isdict = _dict_records(stream)
    j = int(np.flatnonzero(isdict)[len(np.flatnonzero(isdict)) // 2])
    tab = dict_case["tab"].copy()
    hit = np.flatnonzero((tab["block_id"] == recs[j]["block_id"]).all(axis=1))
    assert len(hit) == 1
    tab["index"][hit[0]] += 1000
    path = dict_case["dir"] / "dict-bootstrap-moved"
    path.write_bytes(rafs.write_v6_bootstrap(tab, dict_case["cs"], flags=0x5, blobs=dict_case["blobs"]))
    with nydus_gpu.Engine(chunk_size=dict_case["cs"]) as eng:
        d = eng.dict_open(str(path))
        rep = eng.check(stream, dict=d)
        d.release()
    assert rep["bad"] == rep["dict_bad"] == 1 and _ids(rep) == [_rid(recs[j], "DICT")], rep
    assert rep["dict_checked"] == int(isdict.sum())
    assert rep["bad_list"][0]["expected"] == bytes(recs[j]["block_id"]).hex()


@pytest.mark.parametrize("mode", [nydus_gpu.NODE_DICT_PARTITION, nydus_gpu.NODE_DICT_REPLICATE])
def test_check_on_a_node_with_a_node_dict(dict_case, mode):
    stream = dict_case["oci_lower"]
    recs, isdict = _dict_records(stream)
    node = nydus_gpu.Node([0, 0], chunk_size=dict_case["cs"])
    try:
        d = node.dict_open(dict_case["path"], mode)
        rep = node.check(stream, dict=d)
        d.release()
    finally:
        node.close()
    nd = int(isdict.sum())
    assert nd > 0 and (rep["dict_checked"], rep["dict_bad"], rep["skipped"], rep["bad"]) == (nd, 0, 0, 0), rep
    assert rep["checked"] == len(recs) - nd and rep["records"] == len(recs)


# ---- mismatched engine ------------------------------------------------------------
def test_check_rejects_other_digester_chunk_size_and_targz_ref(streams, tars):
    stream = streams("edge_pax", "none", "blake3")
    for kw in (dict(digester="sha256", chunk_size=S), dict(chunk_size=2 * S)):
        with nydus_gpu.Engine(**kw) as eng:
            with pytest.raises(nydus_gpu.NgpuError) as e:
                eng.check(stream)
            assert e.value.code == nydus_gpu.EINVAL and "inconsistent" in str(e.value), kw
    import gzip
    from nydus_gpu import converter as cv
    out = io.BytesIO()
    w = cv.Pack(out, cv.PackOption(OCIRef=True))
    w.write(gzip.compress(tars["oci_lower"], mtime=0))
    w.close()
    with nydus_gpu.Engine() as eng:
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.check(out.getvalue())
        assert e.value.code == nydus_gpu.EUNSUPP


# ---- CLI ------------------------------------------------------------------------
def test_inspect_check_cli_exit_codes(streams, tmp_path):
    stream = streams("edge_pax", "zstd")
    recs = _records(stream)[1]["chunks"]
    j = 2
    (tmp_path / "clean").write_bytes(stream)
    (tmp_path / "bad").write_bytes(_patch(stream, j, "block_id", lambda d: d ^ np.uint8(1)))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "nydus-snapshotter_amd")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])

    def run(name, *extra):
        return subprocess.run([sys.executable, "-m", "nydus_gpu.inspect", "--check", str(tmp_path / name),
                               *extra], capture_output=True, text=True, timeout=120, env=env)
    r = run("clean")
    assert r.returncode == 0, r.stdout + r.stderr
    rep = json.loads(r.stdout)
    assert rep["bad"] == 0 and rep["checked"] == len(recs)
    r = run("bad", "--chunk-size", hex(S), "--digester", "blake3")
    assert r.returncode == 1, r.stdout + r.stderr
    rep = json.loads(r.stdout)
    assert rep["bad"] == 1 and _ids(rep) == [_rid(recs[j], "DIGEST")]
