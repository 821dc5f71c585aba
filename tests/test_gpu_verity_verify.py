"""Verity verify on the GPU: an image against its STORED dm-verity tree
(ngpu_verity_verify_tree_device / _data_device / _image, csrc/verity.hip)
against the hashlib restatement in tests/verity_verify_oracle.py.

* the device calls: every data-block count at which a wave, a hash block, a
  workgroup or a level begins or ends, bitmaps and counts pre-filled with 0xFF
  and followed by a guard region -- so every word is proven written and nothing
  is stored past the end -- clean images, data damage, tree damage at every
  level, the root, spare areas, a seeded mix, windows, and a four-level image of
  2^21 + 1 blocks gathered on the device;
* argument checks, stream ordering, two streams, the engine's digester;
* the host pipeline: windows, short reads, failing readers, truncated files, a
  tree further on, the order of the findings and the cap;
* verity_file(append=True) -> verity_verify_file, and the command line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nydus_gpu
import verity_oracle as vo
import verity_verify_oracle as vvo
from nydus_gpu._lib import READ_AT_FN

from conftest import ROOT

pytestmark = pytest.mark.gpu

SHAPES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 16383, 16384, 16385, 16514, 32769]
MAX_BLOCKS = max(SHAPES)
GUARD = 4096
CLEAN = ([], [], [])


@pytest.fixture(scope="module")
def eng():
    e = nydus_gpu.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def images():
    """pattern -> (MAX_BLOCKS of data, their leaf digests): every shape is a
    prefix, so each pattern is hashed on the host once."""
    data = {"random": np.random.default_rng(0x7E22).integers(0, 256, MAX_BLOCKS * 512, dtype=np.uint8).tobytes(),
            "zero": bytes(MAX_BLOCKS * 512)}
    return {k: (v, vo.leaf_digests(v)) for k, v in data.items()}


def _clean(images, pattern, blocks):
    data, dig = images[pattern]
    tree, root = vo.tree_from_leaves(dig[:blocks])
    return data[:blocks * 512], tree, root


def _cuda(data):
    if len(data) == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()


def _flip(buf: bytes, *at) -> bytes:
    b = bytearray(buf)
    for i in at:
        b[i] ^= 0x20
    return bytes(b)


class _Out:
    """`words` 64-bit words pre-filled with 0xFF, followed by a guard region."""

    def __init__(self, words):
        self.words = words
        self.t = torch.full((8 * words + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.t.data_ptr()

    def read(self):
        h = self.t.cpu().numpy()
        assert (h[8 * self.words:] == 0xFF).all(), "stored past the end"
        return h[:8 * self.words].view(np.uint64).copy()

    def untouched(self):
        return bool((self.t == 0xFF).all())


def _set_bits(words, n):
    """The set bits of a bitmap of n bits; no bit at or past n may be set."""
    bits = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).tolist()
    assert all(b < n for b in bits), f"bits past {n}: {[b for b in bits if b >= n]}"
    return bits


def _verify_data(eng, d_data, blocks, d_tree, root, first=0, n=None, stream=None):
    """The bad blocks of window [first, first + n) as image block numbers."""
    n = blocks - first if n is None else n
    bm, cnt = _Out((n + 63) // 64), _Out(1)
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream()
    eng.verity_verify_data_device(d_data.data_ptr(), first, n, blocks * 512, d_tree.data_ptr(), root,
                                  bm.ptr(), cnt.ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    bits = _set_bits(bm.read(), n)
    assert int(cnt.read()[0]) == len(bits)
    return [first + k for k in bits]


def _verify_tree(eng, blocks, d_tree, root, stream=None):
    """(tree blocks with a bad hash, levels with a bad spare area)."""
    tb = nydus_gpu.verity_layout(blocks * 512)["tree_bytes"] // 4096
    bm, cnt = _Out((tb + 63) // 64), _Out(2)
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream()
    eng.verity_verify_tree_device(blocks * 512, d_tree.data_ptr(), root, bm.ptr(), cnt.ptr(),
                                  stream=s.cuda_stream)
    torch.cuda.synchronize()
    bits = _set_bits(bm.read(), tb)
    c = cnt.read()
    assert int(c[0]) == len(bits)
    assert int(c[1]) >> 8 == 0
    return bits, [l for l in range(8) if int(c[1]) >> l & 1]


def _verify(eng, data, tree, root):
    """The device calls' verdicts on host buffers, in the oracle's form."""
    blocks = len(data) // 512
    d_data, d_tree = _cuda(data), _cuda(tree)
    bad_hash, spare = _verify_tree(eng, blocks, d_tree, root)
    return _verify_data(eng, d_data, blocks, d_tree, root), bad_hash, spare


# ---- the device calls ------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random", "zero"])
@pytest.mark.parametrize("blocks", SHAPES)
def test_clean_image_has_no_findings(eng, images, pattern, blocks):
    data, tree, root = _clean(images, pattern, blocks)
    assert vvo.verdicts_from_leaves(images[pattern][1][:blocks], tree, root) == CLEAN
    assert _verify(eng, data, tree, root) == CLEAN


def test_tree_shapes_that_cross_a_word_and_a_workgroup():
    # 16514 blocks: 133 tree blocks, three bitmap words, three levels in one launch;
    # 32769 blocks: 261 tree blocks, more than one 256-lane workgroup
    assert nydus_gpu.verity_layout(16514 * 512)["tree_bytes"] == 133 * 4096
    assert nydus_gpu.verity_layout(32769 * 512)["tree_bytes"] == 261 * 4096


@pytest.mark.parametrize("blocks", SHAPES)
def test_data_damage_sets_exactly_those_bits(eng, images, blocks):
    data, tree, root = _clean(images, "random", blocks)
    hit = sorted({b for b in (0, 63, 64, 127, 128, 255, 256, blocks - 1) if b < blocks})
    data = _flip(data, *(512 * b + (37 * b) % 512 for b in hit))
    want = vvo.verdicts(data, tree, root)
    assert want == (hit, [], [])
    assert _verify(eng, data, tree, root) == want


def _tree_damage(kind, data, tree, root):
    blocks = len(data) // 512
    lay = vo.layout(len(data))
    first, sizes = lay["first"], lay["level_blocks"]
    if kind == "level0_slot":
        j, s = sizes[0] // 2, 5 if sizes[0] > 2 else 0
        return data, _flip(tree, (first[0] + j) * 4096 + 32 * s + 9), root
    if kind == "top":
        return data, _flip(tree, 32 + 7), root  # digest slot 1 of the top block
    if kind == "middle":
        assert lay["levels"] >= 3
        return data, _flip(tree, (first[1] + sizes[1] - 1) * 4096 + 1), root  # slot 0 of level 1's last block
    assert kind == "root"
    return data, tree, _flip(root, 31)


@pytest.mark.parametrize("blocks,kind", [(b, k) for b in (129, 16385, 16514)
                                         for k in ("level0_slot", "top", "middle", "root")
                                         if k != "middle" or b > 129] + [(1, "root")])
def test_tree_damage_is_found_where_it_is(eng, images, blocks, kind):
    data, tree, root = _tree_damage(kind, *_clean(images, "random", blocks))
    want = vvo.verdicts(data, tree, root)
    assert want != CLEAN
    if kind == "root":
        assert want == (([0], [], []) if blocks == 1 else ([], [0], []))
    if kind == "level0_slot":  # the hash block that holds the slot, and the slot's data block; nothing above
        assert len(want[0]) == 1 and len(want[1]) == 1 and want[2] == []
    assert _verify(eng, data, tree, root) == want


@pytest.mark.parametrize("blocks", [129, 16514])
def test_spare_area(eng, images, blocks):
    data, tree, root = _clean(images, "random", blocks)
    lay = vo.layout(len(data))
    last0 = lay["first"][0] + lay["level_blocks"][0] - 1
    # not rehashed: the mask bit and the block's bad hash
    d, t, r, want = vvo.damage("spare", data, tree, root)
    assert want == ([], [last0], [0]) and vvo.verdicts(d, t, r) == want
    assert _verify(eng, d, t, r) == want
    # hash-consistent up to a new root: the mask bit alone
    d, t, r, want = vvo.damage("spare_consistent", data, tree, root)
    assert want == ([], [], [0]) and vvo.verdicts(d, t, r) == want
    assert _verify(eng, d, t, r) == want
    # the first spare byte, right behind the last digest
    used = blocks - 128 * (lay["level_blocks"][0] - 1)
    t2 = bytearray(tree)
    t2[last0 * 4096 + 32 * used] = 0x80
    r2 = vvo.rehash_up(t2, blocks, 0, lay["level_blocks"][0] - 1)
    assert _verify(eng, data, bytes(t2), r2) == ([], [], [0]) == vvo.verdicts(data, bytes(t2), r2)
    if lay["levels"] >= 3:  # level 1's last block: 130 - 128 digests used
        t3 = bytearray(tree)
        j = lay["level_blocks"][1] - 1
        t3[(lay["first"][1] + j) * 4096 + 4000] = 7
        r3 = vvo.rehash_up(t3, blocks, 1, j)
        assert _verify(eng, data, bytes(t3), r3) == ([], [], [1]) == vvo.verdicts(data, bytes(t3), r3)


@pytest.mark.parametrize("blocks", [16514, 32769])
def test_random_mix(eng, images, blocks):
    data, tree, root = _clean(images, "random", blocks)
    rng = np.random.default_rng(blocks)
    lay = vo.layout(len(data))
    hit = rng.choice(blocks, blocks // 100, replace=False)
    data = _flip(data, *(512 * int(b) + int(rng.integers(512)) for b in hit))
    slots = []
    for l in range(lay["levels"]):  # a few digest slots of every level
        below = blocks if l == 0 else lay["level_blocks"][l - 1]
        slots += [lay["first"][l] * 4096 + 32 * int(c) + int(rng.integers(32))
                  for c in rng.choice(below, min(3, below), replace=False)]
    tree = _flip(tree, *set(slots))
    want = vvo.verdicts(data, tree, root)
    assert len(want[0]) >= blocks // 100 and len(want[1]) >= 3
    assert _verify(eng, data, tree, root) == want


def test_windows(eng, images):
    blocks = 16514
    data, tree, root = _clean(images, "random", blocks)
    rng = np.random.default_rng(3)
    hit = sorted(set(rng.choice(blocks, 300, replace=False).tolist()) | {64, 65, 128, 264, 265, 16383, blocks - 1})
    data = _flip(data, *(512 * b + 3 for b in hit))
    tree = _flip(tree, (3 + 1) * 4096 + 32 * 2)  # the stored digest of data block 130
    want = vvo.verdicts(data, tree, root)[0]
    assert 130 in want
    d_data, d_tree = _cuda(data), _cuda(tree)
    for first, n in ((65, 200), (blocks - 1, 1), (128, 16384 - 128), (0, blocks)):
        win = d_data[first * 512:(first + n) * 512]
        assert win.data_ptr() % 16 == 0
        got = _verify_data(eng, win, blocks, d_tree, root, first=first, n=n)
        assert got == [b for b in want if first <= b < first + n], (first, n)


def test_four_levels(eng):
    """2^21 + 1 data blocks: levels of 16385 / 129 / 2 / 1 hash blocks, gathered
    on the device from 257 distinct blocks; the tree comes from
    ngpu_verity_device.  Damage: the last data block, one level-1 digest, one
    level-2 byte."""
    n = 2 ** 21 + 1
    rng = np.random.default_rng(0x4C5)
    table = rng.integers(0, 256, (257, 512), dtype=np.uint8)
    idx = rng.integers(0, 257, n)
    idx[:257] = np.arange(257)
    d_data = _cuda(table.tobytes()).view(257, 512).index_select(0, torch.from_numpy(idx).cuda()).reshape(-1)
    lay = vo.layout(n * 512)
    assert lay["level_blocks"] == [16385, 129, 2, 1] and lay["first"] == [132, 3, 1, 0]
    d_tree = torch.empty(lay["tree_bytes"], dtype=torch.uint8, device="cuda")
    d_root = torch.empty(32, dtype=torch.uint8, device="cuda")
    eng.verity_device(d_data.data_ptr(), n * 512, d_tree.data_ptr(), d_root.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    root = d_root.cpu().numpy().tobytes()
    dig = vo.leaf_digests(table.tobytes())[idx]
    assert _verify_tree(eng, n, d_tree, root) == ([], [])
    assert _verify_data(eng, d_data, n, d_tree, root) == []
    at1 = (3 + 5) * 4096 + 32 * 7 + 3   # level 1, block 5, slot 7
    at2 = (1 + 0) * 4096 + 32 * 9 + 30  # level 2, block 0, slot 9
    d_data[(n - 1) * 512 + 100] ^= 0x04
    d_tree[at1] ^= 0x04
    d_tree[at2] ^= 0x04
    import hashlib
    last = bytearray(table[idx[-1]].tobytes())
    last[100] ^= 0x04
    dig = dig.copy()
    dig[-1] = np.frombuffer(hashlib.sha256(last).digest(), np.uint8)
    want = vvo.verdicts_from_leaves(dig, d_tree.cpu().numpy().tobytes(), root)
    assert want == ([n - 1], [1, 3 + 5, 3 + 9, 132 + 128 * 5 + 7], [])
    assert (_verify_data(eng, d_data, n, d_tree, root), *_verify_tree(eng, n, d_tree, root)) == want


def test_rejected_calls_launch_nothing(eng, images):
    blocks = 129
    data, tree, root = _clean(images, "random", blocks)
    base = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    base[:len(data)] = _cuda(data)
    d_tree = _cuda(tree)
    bm, cnt, tbm, tcnt = _Out(3), _Out(1), _Out(1), _Out(2)
    s = torch.cuda.current_stream().cuda_stream
    nb = blocks * 512
    D, T = base.data_ptr(), d_tree.data_ptr()
    for dd, first, n, nbytes, dt, b, c in ((D + 4, 0, blocks, nb, T, bm.ptr(), cnt.ptr()),
                                           (D, 0, blocks, nb, T + 4, bm.ptr(), cnt.ptr()),
                                           (D, 0, blocks, nb, T, bm.ptr() + 4, cnt.ptr()),
                                           (D, 0, blocks, nb, T, bm.ptr(), cnt.ptr() + 4),
                                           (D, 0, blocks, 0, T, bm.ptr(), cnt.ptr()),
                                           (D, 0, blocks, nb - 1, T, bm.ptr(), cnt.ptr()),
                                           (D, 0, blocks + 1, nb, T, bm.ptr(), cnt.ptr()),
                                           (D, 100, 30, nb, T, bm.ptr(), cnt.ptr()),
                                           (D, blocks + 1, 0, nb, T, bm.ptr(), cnt.ptr()),
                                           (D, 2 ** 63, 2 ** 63 + 1, nb, T, bm.ptr(), cnt.ptr()),
                                           (D, 0, blocks, nb, 0, bm.ptr(), cnt.ptr())):
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.verity_verify_data_device(dd, first, n, nbytes, dt, root, b, c, stream=s)
        assert e.value.code == nydus_gpu.EINVAL, (dd, first, n, nbytes, dt)
    for nbytes, dt, b, c in ((nb, T + 4, tbm.ptr(), tcnt.ptr()), (nb, T, tbm.ptr() + 4, tcnt.ptr()),
                             (nb, T, tbm.ptr(), tcnt.ptr() + 4), (0, T, tbm.ptr(), tcnt.ptr()),
                             (nb + 1, T, tbm.ptr(), tcnt.ptr()), (nb, 0, tbm.ptr(), tcnt.ptr())):
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.verity_verify_tree_device(nbytes, dt, root, b, c, stream=s)
        assert e.value.code == nydus_gpu.EINVAL, (nbytes, dt)
    with pytest.raises(ValueError):
        eng.verity_verify_tree_device(nb, T, root[:31], tbm.ptr(), tcnt.ptr(), stream=s)
    torch.cuda.synchronize()
    assert bm.untouched() and cnt.untouched() and tbm.untouched() and tcnt.untouched(), \
        "a rejected call launched something"
    # nothing to do: the counts are zeroed, nothing else is written
    eng.verity_verify_data_device(D, 5, 0, nb, T, root, bm.ptr(), cnt.ptr(), stream=s)
    eng.verity_verify_tree_device(512, 0, root, 0, tcnt.ptr(), stream=s)  # one data block: no tree
    torch.cuda.synchronize()
    assert bm.untouched() and tbm.untouched()
    assert cnt.read().tolist() == [0] and tcnt.read().tolist() == [0, 0]
    eng.device_status()


def test_result_does_not_depend_on_the_digester(images):
    data, tree, root = _clean(images, "random", 257)
    data = _flip(data, 512 * 200)
    tree = _flip(tree, 4096 + 32 * 2)
    want = vvo.verdicts(data, tree, root)
    for digester in ("blake3", "sha256"):
        with nydus_gpu.Engine(digester=digester) as e:
            assert _verify(e, data, tree, root) == want, digester
            assert e.verity_verify(data, tree, root)["bad"] == len(want[0]) + len(want[1]), digester


def test_verify_is_ordered_on_the_callers_stream(eng, images):
    """The image and its tree are produced on the caller's (non-default) stream
    right before the calls, behind a few milliseconds of other work: a kernel on
    any other stream would see the zeros the buffers held and call every block
    bad."""
    blocks = MAX_BLOCKS
    data, tree, root = _clean(images, "random", blocks)
    data = _flip(data, 512 * 777 + 1)
    src, src_tree = _cuda(data), _cuda(tree)
    d_data = torch.zeros(blocks * 512, dtype=torch.uint8, device="cuda")
    d_tree = torch.zeros(len(tree), dtype=torch.uint8, device="cuda")
    bm, cnt, tbm, tcnt = _Out((blocks + 63) // 64), _Out(1), _Out((len(tree) // 4096 + 63) // 64), _Out(2)
    x = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            x = x @ x * 1e-3
        d_data.copy_(src)
        d_tree.copy_(src_tree)
        eng.verity_verify_data_device(d_data.data_ptr(), 0, blocks, blocks * 512, d_tree.data_ptr(), root,
                                      bm.ptr(), cnt.ptr(), stream=s.cuda_stream)
        eng.verity_verify_tree_device(blocks * 512, d_tree.data_ptr(), root, tbm.ptr(), tcnt.ptr(),
                                      stream=s.cuda_stream)
    s.synchronize()
    assert _set_bits(bm.read(), blocks) == [777] and cnt.read().tolist() == [1]
    assert _set_bits(tbm.read(), len(tree) // 4096) == [] and tcnt.read().tolist() == [0, 0]


def test_two_images_on_two_streams(eng, images):
    jobs = []
    for pattern, blocks, hit in (("random", MAX_BLOCKS, 31000), ("zero", 16385, 5)):
        data, tree, root = _clean(images, pattern, blocks)
        data = _flip(data, 512 * hit)
        jobs.append((torch.cuda.Stream(), _cuda(data), _cuda(tree), root, blocks, hit,
                     _Out((blocks + 63) // 64), _Out(1), _Out((len(tree) // 4096 + 63) // 64), _Out(2)))
    torch.cuda.synchronize()
    for _ in range(3):  # both streams hold several calls at once
        for s, d, t, root, blocks, hit, bm, cnt, tbm, tcnt in jobs:
            eng.verity_verify_tree_device(blocks * 512, t.data_ptr(), root, tbm.ptr(), tcnt.ptr(),
                                          stream=s.cuda_stream)
            eng.verity_verify_data_device(d.data_ptr(), 0, blocks, blocks * 512, t.data_ptr(), root,
                                          bm.ptr(), cnt.ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    for s, d, t, root, blocks, hit, bm, cnt, tbm, tcnt in jobs:
        assert _set_bits(bm.read(), blocks) == [hit] and cnt.read().tolist() == [1]
        assert _set_bits(tbm.read(), t.numel() // 4096) == [] and tcnt.read().tolist() == [0, 0]
    eng.device_status()


# ---- the host pipeline -----------------------------------------------------------------
IMG_BLOCKS = 16514


def _reader(src, calls=None, short=0, fail_from=None):
    """A READ_AT_FN over bytes: `short` caps what one call returns, reads that
    reach `fail_from` fail, `calls` collects (offset, bytes returned)."""
    buf = np.frombuffer(src, np.uint8)

    def ra(_ctx, dst, n, off):
        n = min(n, buf.size - off)
        if short:
            n = min(n, short)
        if n <= 0 or (fail_from is not None and off + n > fail_from):
            return -1
        ctypes.memmove(dst, buf.ctypes.data + off, n)
        if calls is not None:
            calls.append((off, n))
        return n
    return READ_AT_FN(ra)


def _file(data, tree, extra=0):
    """data, zeros up to the hash offset (+ extra), the tree."""
    off = vo.layout(len(data))["hash_offset"] + extra
    return data + bytes(off - len(data)) + tree, off


@pytest.fixture(scope="module")
def damaged(images):
    """A 16514-block image with findings of every kind: (data, tree, root,
    verdicts)."""
    data, tree, root = _clean(images, "random", IMG_BLOCKS)
    lay = vo.layout(len(data))
    data = _flip(data, *(512 * b + 11 for b in (0, 2047, 2048, 9000, 16384, IMG_BLOCKS - 1)))
    # a level-0 slot, a level-1 slot, a slot of the top block
    t = bytearray(_flip(tree, (3 + 77) * 4096 + 32 * 3, 4096 + 32 * 1 + 4, 32 * 1 + 2))
    t[(3 + 129) * 4096 + 4095] = 9   # level 0's spare area, not rehashed
    t[2 * 4096 + 2000] = 1           # level 1's spare area, not rehashed
    found = vvo.verdicts(data, bytes(t), root)
    assert found == ([0, 2047, 2048, 9000, 128 * 77 + 3, 16384, IMG_BLOCKS - 1],
                     [0, 1, 2, 3 + 1, 3 + 77, 3 + 129], [0, 1]) and lay["first"] == [3, 1, 0]
    return data, bytes(t), root, found


def _report(found, blocks, tree_len, hash_offset, cap=64):
    lay = vo.layout(blocks * 512)
    full = vvo.findings(found, blocks, hash_offset)
    return {"data_blocks": blocks, "tree_blocks": tree_len // 4096, "levels": lay["levels"],
            "bad_data": len(found[0]), "bad_hash": len(found[1]), "bad_spare": len(found[2]),
            "bad": len(full), "bytes": blocks * 512 + tree_len, "bad_list": full[:cap]}


def test_image_windows_equal_the_oracle(eng, images, damaged):
    data, tree, root, found = damaged
    img, off = _file(data, tree)
    want = _report(found, IMG_BLOCKS, len(tree), off)
    assert eng.verity_verify(data, tree, root) == {**want, "bad_list": vvo.findings(found, IMG_BLOCKS, len(data))}
    # 1 MiB: 8 windows and a ragged one; 2047 blocks: a window that ends right
    # before a damaged block; 1,000,000: not a multiple of 512 (1953 blocks);
    # 100 blocks: the tree takes eleven windows; 0: one window for all
    for window in (1 << 20, 2047 * 512, 1000000, 100 * 512, 0):
        calls = []
        got = eng.verity_verify_image(_reader(img, calls), len(data), off, root, window_bytes=window)
        assert got == want, window
        assert sum(n for _, n in calls) == len(data) + len(tree), window
        if not window:
            continue
        w = window - window % 512
        # every byte read once, no read across a window; the tree first, then the data
        assert sorted(calls) == sorted([(at, min(w, len(data) - at)) for at in range(0, len(data), w)] +
                                       [(off + at, min(w, len(tree) - at)) for at in range(0, len(tree), w)])
        assert min(i for i, c in enumerate(calls) if c[0] < off) == len(range(0, len(tree), w)), window
    clean = _clean(images, "random", IMG_BLOCKS)
    img, off = _file(clean[0], clean[1])
    assert eng.verity_verify_image(_reader(img), len(clean[0]), off, clean[2], window_bytes=1 << 20) == \
        _report(CLEAN, IMG_BLOCKS, len(tree), off)
    for blocks in (1, 2, 129):  # no tree at all; a tree larger than the data
        d, t, r = _clean(images, "zero", blocks)
        img, off = _file(d, t)
        assert eng.verity_verify_image(_reader(img), len(d), off, r) == _report(CLEAN, blocks, len(t), off)
        assert eng.verity_verify_image(_reader(img), len(d), off, _flip(r, 0))["bad_list"] == \
            vvo.findings(([0], [], []) if blocks == 1 else ([], [0], []), blocks, off)


def test_image_reader_with_short_reads(eng, damaged):
    data, tree, root, found = damaged
    img, off = _file(data, tree)
    calls = []
    got = eng.verity_verify_image(_reader(img, calls, short=4099), len(data), off, root,
                                  window_bytes=3 << 20, threads=3)
    assert got == _report(found, IMG_BLOCKS, len(tree), off)
    assert max(n for _, n in calls) == 4099 and sum(n for _, n in calls) == len(data) + len(tree)


def test_image_tree_further_on(eng, damaged):
    data, tree, root, found = damaged
    img, off = _file(data, tree, extra=3 * 4096)
    assert off == vo.layout(len(data))["hash_offset"] + 3 * 4096
    assert eng.verity_verify_image(_reader(img), len(data), off, root, window_bytes=1 << 20) == \
        _report(found, IMG_BLOCKS, len(tree), off)


def test_image_errors_release_everything(eng, images):
    data, tree, root = _clean(images, "random", IMG_BLOCKS)
    img, off = _file(data, tree)
    window = 1 << 20
    ok = eng.verity_verify_image(_reader(img), len(data), off, root, window_bytes=window)
    assert ok["bad"] == 0
    free0 = torch.cuda.mem_get_info()[0]
    before = eng.counters()
    # in the tree, in the last data window, in the middle, at once
    for fail_from in (off + 4096 + 1, len(data) - 1, 5 * window + 77, 1):
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.verity_verify_image(_reader(img, fail_from=fail_from), len(data), off, root, window_bytes=window)
        assert e.value.code == nydus_gpu.EIO, fail_from
        assert eng.counters() == before, fail_from
    # a file that ends inside the tree, and one that ends before it
    for cut in (off + len(tree) - 1, off + 4096, off, len(data)):
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.verity_verify_image(_reader(img[:cut]), len(data), off, root, window_bytes=window)
        assert e.value.code == nydus_gpu.EIO, cut
        assert eng.counters() == before, cut
    for args in ((len(data), len(data) - 512), (len(data), 0), (len(data) - 1, off), (0, off),
                 (len(data), 2 ** 64 - 4096)):
        with pytest.raises(nydus_gpu.NgpuError) as e:
            eng.verity_verify_image(_reader(img), args[0], args[1], root, window_bytes=window)
        assert e.value.code == nydus_gpu.EINVAL, args
    with pytest.raises(nydus_gpu.NgpuError) as e:
        eng.verity_verify_image(_reader(img), len(data), off, root, window_bytes=511)
    assert e.value.code == nydus_gpu.EINVAL
    assert eng.counters() == before
    assert torch.cuda.mem_get_info()[0] >= free0, "device memory was not given back"
    assert eng.verity_verify_image(_reader(img), len(data), off, root, window_bytes=window) == ok
    eng.device_status()


def test_image_findings_order_and_cap(eng, damaged):
    data, tree, root, found = damaged
    img, off = _file(data, tree)
    full = vvo.findings(found, IMG_BLOCKS, off)
    assert [(f["reason"], f["block"]) for f in full[:9]] == \
        [("HASH", 0), ("HASH", 1), ("HASH", 2), ("SPARE", 2), ("HASH", 4), ("HASH", 80), ("HASH", 132),
         ("SPARE", 132), ("DATA", 0)]
    for cap in (0, 1, 3, 4, 8, 9, len(full), len(full) + 5):
        for window in (0, 1 << 20):
            got = eng.verity_verify_image(_reader(img), len(data), off, root, max_bad=cap, window_bytes=window)
            assert got == _report(found, IMG_BLOCKS, len(tree), off, cap), (cap, window)


# ---- files and the command line --------------------------------------------------------------
def test_verity_file_then_verify_file(eng, images, tmp_path):
    data = images["random"][0][:1001 * 512]  # 3584 bytes of padding before the tree
    path = str(tmp_path / "disk.img")
    with open(path, "wb") as f:
        f.write(data)
    info = eng.verity_file(path, append=True)
    rep = eng.verity_verify_file(path, info["data_blocks"], info["hash_offset"], info["root"])
    assert rep == _report(CLEAN, 1001, info["tree_bytes"], info["hash_offset"])
    v = nydus_gpu.parse_verity_label(nydus_gpu.verity_label(info))
    assert eng.verity_verify_file(path, v["data_blocks"], v["hash_offset"], bytes.fromhex(v["root"])) == rep
    with open(path, "r+b") as f:  # the file ends inside the tree
        f.truncate(info["hash_offset"] + info["tree_bytes"] - 100)
    with pytest.raises(nydus_gpu.NgpuError) as e:
        eng.verity_verify_file(path, info["data_blocks"], info["hash_offset"], info["root"])
    assert e.value.code == nydus_gpu.EIO


CLI_BLOCKS = 1001  # level 0: 8 hash blocks (tree blocks 1..8), level 1: tree block 0


def _cli(*args):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "nydus-snapshotter_amd")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    return subprocess.run([sys.executable, "-m", "nydus_gpu.inspect", *args], capture_output=True,
                          text=True, timeout=120, env=env)


def _main(capsys, *args):
    """nydus_gpu.inspect's main() in this process: (exit code, stdout)."""
    from nydus_gpu import inspect
    capsys.readouterr()
    try:
        rc = inspect.main(list(args))
    except SystemExit as e:  # argparse's usage error
        rc = e.code
    return rc, capsys.readouterr().out


def test_inspect_verity_scan(images, tmp_path, capsys):
    """Two runs as a process (a clean file: 0; a damaged one: 1); the other
    cases through the same main() in this process, which costs no interpreter
    start each."""
    data = images["random"][0][:CLI_BLOCKS * 512]
    clean = vo.image_file(data)
    off, root = vo.layout(len(data))["hash_offset"], vo.tree(data)[1].hex()
    tree_len = len(clean) - off
    path = tmp_path / "disk.img"
    three = ("--data-blocks", str(CLI_BLOCKS), "--hash-offset", str(off), root)
    label = ("--label", f"{CLI_BLOCKS},{off},sha256:{root}")

    def scan(content, *how, process=False):
        path.write_bytes(content)
        if process:
            r = _cli("--verity-scan", str(path), *how)
            rc, out = r.returncode, r.stdout
        else:
            rc, out = _main(capsys, "--verity-scan", str(path), *how)
        assert rc in (0, 1), out
        return rc, json.loads(out)

    def old(content):
        path.write_bytes(content)
        return _main(capsys, "--verity-verify", str(path), *three)[0]

    assert scan(clean, *three, process=True) == (0, _report(CLEAN, CLI_BLOCKS, tree_len, off))
    assert scan(clean, *label) == (0, _report(CLEAN, CLI_BLOCKS, tree_len, off))
    assert old(clean) == 0
    # one data byte: exactly that block, and no hash block
    bad = _flip(clean, 700 * 512 + 13)
    want = _report(([700], [], []), CLI_BLOCKS, tree_len, off)
    assert want["bad_data"] == 1 and want["bad_list"][0]["block"] == 700
    assert scan(bad, *label, process=True) == (1, want)
    assert scan(bad, *three) == (1, want)
    assert old(bad) == 1
    # one byte of tree block 3 = level-0 hash block 2, digest slot 3: the block,
    # what it covers, and the slot's data block
    bad = _flip(clean, off + 3 * 4096 + 100)
    want = _report(([2 * 128 + 3], [3], []), CLI_BLOCKS, tree_len, off)
    assert want["bad_list"][0] == {"reason": "HASH", "level": 0, "block": 3, "first_data_block": 256,
                                   "last_data_block": 383, "file_offset": off + 3 * 4096}
    assert scan(bad, *label) == (1, want)
    assert scan(bad, *three) == (1, want)
    assert old(bad) == 1
    # usage and I/O errors
    path.write_bytes(clean)
    for how in ((), ("--data-blocks", str(CLI_BLOCKS), root), three + label, ("--label", "nonsense"),
                ("--label", f"{CLI_BLOCKS},{off},sha256:{root[:-1]}"), three[:-1] + ("zz",)):
        assert _main(capsys, "--verity-scan", str(path), *how) == (2, ""), how
    path.write_bytes(clean[:-1])
    assert _main(capsys, "--verity-scan", str(path), *label) == (2, "")
    assert _main(capsys, "--verity-scan", str(tmp_path / "missing.img"), *label) == (2, "")
