"""The SHA-256 digest stage's whole dispatch matrix, bit-exact against hashlib:
all seven kernels of csrc/sha256.hip (sha256_split, sha256_lane,
sha256_pair<1,U>, <1,M>, <2,U>, <2,M>, <4,M>) on ragged waves, padding edges at
every lane position, the auto thresholds, what the digest stage may write, and
the kernels' own bad-descriptor branches.  The layers, the Python mirror of the
selection rule (csrc/sha256_plan.hpp) and the CPU proof of which kernel each
call selects are in sha_shapes.py / test_sha_shapes.py; the kernel a call ran is
read back from the bad-descriptor message.  Run on a gfx950 box: pytest -m gpu."""
import re

import numpy as np
import pytest

import nydus_gpu

import sha_shapes as ss

pytestmark = pytest.mark.gpu

VARIANT_FLAGS = [0, 1 << 11, 2 << 11, 3 << 11, 5 << 11, 6 << 11]
DEDUP_FIELDS = ("kind", "index", "ref")
GUARD_ROWS = 128
FILL = 0xA5
assert VARIANT_FLAGS == ss.VARIANT_FLAGS


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(chunk_size, flags):
        k = (chunk_size, flags)
        if k not in cache:
            cache[k] = nydus_gpu.Engine(digester="sha256", chunk_size=chunk_size, flags=flags)
        return cache[k]
    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def refs(oracle):
    """(layer, pad) -> bytes, chunks, chunk size, hashlib digests and the
    oracle's dedup decisions: computed once and only read by the tests."""
    out = {}
    for layer, pad in (("E", True), ("E", False), ("R", True), ("R", False), ("C", False)):
        build, chunk_size = ss.LAYERS[layer]
        data, ch = build(pad)
        dig = ss.hashlib_digests(data, ch)
        dec, _ = oracle.dedup(dig, ch["length"])
        assert ((dec["kind"] == nydus_gpu.INTRA) & (ch["length"] > 8)).sum() >= 4  # the planted duplicates
        for a in (ch, dig, dec):
            a.setflags(write=False)
        out[(layer, pad)] = (data, ch, chunk_size, dig, dec)
    return out


def _where(ch, bad):
    ids = [int(i) for i in bad[:8]]
    return (f"{len(bad)} bad chunks, first ids={ids} lengths={[int(ch['length'][i]) for i in ids]} "
            f"offset%16={[int(ch['offset'][i]) % 16 for i in ids]} index%32={[i % 32 for i in ids]}")


def _tag(layer, pad, n, flags, data, chunk_size):
    return (f"layer {layer} {'padded' if pad else 'plain'} n={n} flags={flags:#x} "
            f"(variant {ss.variant_of(flags)}, {ss.pick_name(flags, n, len(data), chunk_size)})")


def _process_and_compare(engines, oracle, refs, layer, pad, n, flags):
    data, ch, chunk_size, dig, dec = refs[(layer, pad)]
    tag = _tag(layer, pad, n, flags, data, chunk_size)
    if n != len(ch):
        dec, _ = oracle.dedup(dig[:n], ch["length"][:n])
    out, st = engines(chunk_size, flags).process(data, ch[:n])
    bad = np.nonzero((out["digest"] != dig[:n]).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: digest: {_where(ch, bad)}"
    for f in DEDUP_FIELDS:
        bad = np.nonzero(out[f] != dec[f][:n])[0]
        assert bad.size == 0, f"{tag}: {f}: {_where(ch, bad)}"
    assert st["chunks"] == n, tag


def test_every_kernel_vs_hashlib(engines, oracle, refs):
    """Layers E and R, padded (sha_mixed false) and plain (true), under every
    flag through Engine.process: each of the seven kernels on waves whose lanes
    finish at different blocks -- the masked pair kernels too, which calls of
    equal full chunks never show a ragged wave."""
    ran = set()
    for layer in ("E", "R"):
        for pad in (True, False):
            data, ch, chunk_size, _, _ = refs[(layer, pad)]
            for flags in VARIANT_FLAGS:
                ran.add(ss.pick_name(flags, len(ch), len(data), chunk_size))
    assert ran == set(ss.KERNELS), ran  # on the CPU side, before anything runs
    for layer in ("E", "R"):
        for pad in (True, False):
            for flags in VARIANT_FLAGS:
                _process_and_compare(engines, oracle, refs, layer, pad, len(refs[(layer, pad)][1]), flags)


def test_prefixes_and_auto_thresholds(engines, oracle, refs):
    """Layer R cut to 1, 33 and 223 chunks under every flag (a lone lane, one
    chunk past a group, one short of seven groups); layer C under auto on both
    sides of 16384 and 32768 chunks, and its 32,769 chunks under every forced
    flag: many workgroups and a last partial one in every kernel."""
    for n in ss.R_PREFIXES:
        for flags in VARIANT_FLAGS:
            _process_and_compare(engines, oracle, refs, "R", False, n, flags)
    for n in ss.C_PREFIXES:
        _process_and_compare(engines, oracle, refs, "C", False, n, 0)
    for flags in VARIANT_FLAGS[1:]:
        _process_and_compare(engines, oracle, refs, "C", False, ss.C_CHUNKS, flags)


def _digest_on_device(eng, data, ch):
    """ngpu_digest_device over torch buffers, d_out = n + GUARD_ROWS rows of 0xA5.
    -> the rows as uint8 [n + GUARD_ROWS, 64], after a synchronize."""
    import torch
    n = len(ch)
    d_data = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_ch = torch.from_numpy(np.ascontiguousarray(ch).view(np.uint8).copy()).cuda()
    d_out = torch.full(((n + GUARD_ROWS) * 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    eng.digest_device(d_data.data_ptr(), d_data.numel(), d_ch.data_ptr(), n, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out, d_out.cpu().numpy().reshape(n + GUARD_ROWS, 64)


def _check_rows(rows, ch, dig, skip, tag):
    """Rows < n not in `skip`: the digest, kind = DIGESTED, the other 28 bytes
    untouched.  Rows in `skip` and the guard rows: untouched."""
    n = len(ch)
    keep = np.ones(n, bool)
    keep[list(skip)] = False
    bad = np.nonzero(keep & (rows[:n, :32] != dig).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: digest: {_where(ch, bad)}"
    kind = np.ascontiguousarray(rows[:n, 32:36]).view("<u4")[:, 0]
    bad = np.nonzero(keep & (kind != nydus_gpu.DIGESTED))[0]
    assert bad.size == 0, f"{tag}: kind: {_where(ch, bad)}"
    bad = np.nonzero(keep & (rows[:n, 36:] != FILL).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: bytes 36..63 written: {_where(ch, bad)}"
    bad = np.nonzero(~keep & (rows[:n] != FILL).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: row of a refused descriptor written: {_where(ch, bad)}"
    bad = np.nonzero((rows[n:] != FILL).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: guard rows {(bad[:8] + n).tolist()} written"


def test_digest_stage_writes_only_digest_and_kind(engines, refs):
    """Layer E through ngpu_digest_device: 36 bytes of every row below n, and
    nothing past them -- the absent groups of pair<4>'s last workgroup, the tail
    lanes of sha256_lane, the half-row stores of the pair kernels' lane pairs."""
    for pad in (True, False):
        data, ch, chunk_size, dig, _ = refs[("E", pad)]
        for flags in VARIANT_FLAGS:
            eng = engines(chunk_size, flags)
            _, rows = _digest_on_device(eng, data, ch)
            eng.device_status()
            _check_rows(rows, ch, dig, (), _tag("E", pad, len(ch), flags, data, chunk_size))


def test_bad_descriptors_reach_the_kernels(engines, refs):
    """Five refused descriptors per call, in the kernels' own branches (the
    host path would stop them before the launch): the first lane pair, the first
    of the second DPP row, the last lane pair, the next group, the last chunk.  Each kernel
    counts every one exactly once, writes nothing into its row, and digests its
    neighbours.  The message names the kernel: the flag bits and sha_mixed reached
    the launch."""
    for pad in (True, False):
        data, good, chunk_size, dig, _ = refs[("E", pad)]
        n, size = len(good), len(data)
        ch = good.copy()
        bad_ids = [0, 8, 31, 40, n - 1]
        ch["offset"][0] = size + 1                            # starts past the buffer
        ch["offset"][8] = size - int(ch["length"][8]) + 1     # ends one byte past it
        ch["length"][31] = 0xFFFFFFFF                         # a valid offset, a length no buffer holds
        ch["offset"][40] = 1 << 63                            # offset + length would wrap
        ch["offset"][n - 1], ch["length"][n - 1] = size, 1    # starts at the end, one byte long
        for flags in VARIANT_FLAGS:
            tag = _tag("E", pad, n, flags, data, chunk_size)
            eng = engines(chunk_size, flags)
            eng.device_status()
            _, rows = _digest_on_device(eng, data, ch)
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                eng.device_status()
            msg = str(ei.value)
            assert ei.value.code == nydus_gpu.EINVAL, f"{tag}: {msg}"
            assert re.search(r"(?<!\d)5 chunk descriptor\(s\) outside the data buffer", msg), f"{tag}: {msg}"
            name = ss.pick_name(flags, n, size, chunk_size)
            assert f"(digest stage: sha256 {name}, {n} chunks)" in msg, f"{tag}: {msg}"
            eng.device_status()  # cleared by the check
            _check_rows(rows, good, dig, bad_ids, tag)
