"""Verity on the CPU: the geometry of the dm-verity tree (ngpu_verity_layout,
csrc/verity_plan.hpp) against the hashlib restatement in tests/verity_oracle.py,
the restatement against its known answers (tests/golden/verity.json) and, where
libcryptsetup can be loaded, against cryptsetup's own tree; and the stand-alone
sanitizer program over verity_plan.hpp (tests/cpp/verity_plan_test.cpp).  No GPU."""
import ctypes
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import nydus_gpu
import verity_oracle as vo

from conftest import GOLDEN, ROOT


def test_docs_example_geometry():
    # docs/tarfs.md:119-145 of the reference: 194,518,016 data bytes, hash
    # offset 194,519,040, the file with its tree 206,782,464 bytes
    lay = vo.layout(379918 * 512)
    assert lay["levels"] == 3 and lay["level_blocks"] == [2969, 24, 1]
    assert lay["hash_offset"] == 194519040 and lay["tree_bytes"] == 12263424
    assert lay["hash_offset"] + lay["tree_bytes"] == 206782464
    assert lay["first"] == [25, 1, 0]
    got = nydus_gpu.verity_layout(379918 * 512)
    assert got == {"data_blocks": 379918, "hash_offset": 194519040, "tree_bytes": 12263424, "levels": 3,
                   "root": "00" * 32}


EDGES = {1: (0, []), 2: (1, [1]), 128: (1, [1]), 129: (2, [2, 1]), 16384: (2, [128, 1]),
         16385: (3, [129, 2, 1]), 2 ** 21: (3, [16384, 128, 1]), 2 ** 21 + 1: (4, [16385, 129, 2, 1])}


@pytest.mark.parametrize("blocks", sorted(EDGES))
def test_edge_shapes(blocks):
    levels, sizes = EDGES[blocks]
    lay = vo.layout(blocks * 512)
    assert (lay["levels"], lay["level_blocks"]) == (levels, sizes)
    assert lay["tree_bytes"] == 4096 * sum(sizes) and lay["hash_offset"] == -(-blocks * 512 // 4096) * 4096
    got = nydus_gpu.verity_layout(blocks * 512)
    assert (got["data_blocks"], got["levels"], got["tree_bytes"], got["hash_offset"]) == \
        (blocks, levels, lay["tree_bytes"], lay["hash_offset"])


@pytest.mark.parametrize("size", [0, 511, 513, 4095])
def test_layout_rejects_sizes_that_are_not_whole_blocks(size):
    info = nydus_gpu._lib.NgpuVerityInfo()
    assert nydus_gpu.lib().ngpu_verity_layout(size, ctypes.byref(info)) == nydus_gpu.EINVAL
    assert nydus_gpu.lib().ngpu_verity_layout(512, None) == nydus_gpu.EINVAL
    with pytest.raises(nydus_gpu.NgpuError) as e:
        nydus_gpu.verity_layout(size)
    assert e.value.code == nydus_gpu.EINVAL
    with pytest.raises(ValueError):
        vo.layout(size)


def test_layout_equals_the_oracle_for_random_sizes():
    rng = random.Random(0x7E217)
    sizes = [rng.randrange(1, 1 << rng.randrange(1, 53)) for _ in range(4000)]
    sizes += [128 ** k + d for k in range(1, 8) for d in (-1, 0, 1)] + [(1 << 53) - 1]
    for n in sizes:
        lay, got = vo.layout(n * 512), nydus_gpu.verity_layout(n * 512)
        assert (got["data_blocks"], got["levels"], got["tree_bytes"], got["hash_offset"]) == \
            (n, lay["levels"], lay["tree_bytes"], lay["hash_offset"]), n
    info = nydus_gpu._lib.NgpuVerityInfo()
    assert nydus_gpu.lib().ngpu_verity_layout(1 << 62, ctypes.byref(info)) == nydus_gpu.EINVAL


def test_known_answers():
    with open(os.path.join(GOLDEN, "verity.json")) as f:
        rows = json.load(f)["rows"]
    assert [r["data_blocks"] for r in rows] == [1, 129, 16385]
    for r in rows:
        data = vo.pattern(r["data_blocks"])
        lay = vo.layout(len(data))
        tree, root = vo.tree(data)
        assert (lay["levels"], lay["hash_offset"], lay["tree_bytes"]) == \
            (r["levels"], r["hash_offset"], r["tree_bytes"])
        assert root.hex() == r["root"] and len(tree) == r["tree_bytes"]
        assert (hashlib.sha256(tree).hexdigest() if tree else None) == r["tree_sha256"]
    assert nydus_gpu.verity_label({"data_blocks": 129, "hash_offset": 69632, "root": rows[1]["root"]}) == \
        "129,69632,sha256:" + rows[1]["root"]


class _VerityParams(ctypes.Structure):  # struct crypt_params_verity (libcryptsetup.h)
    _fields_ = [("hash_name", ctypes.c_char_p), ("data_device", ctypes.c_char_p),
                ("hash_device", ctypes.c_char_p), ("fec_device", ctypes.c_char_p),
                ("salt", ctypes.c_void_p), ("salt_size", ctypes.c_uint32), ("hash_type", ctypes.c_uint32),
                ("data_block_size", ctypes.c_uint32), ("hash_block_size", ctypes.c_uint32),
                ("data_size", ctypes.c_uint64), ("hash_area_offset", ctypes.c_uint64),
                ("fec_area_offset", ctypes.c_uint64), ("fec_roots", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def cryptsetup():
    try:
        L = ctypes.CDLL("libcryptsetup.so.12")
    except OSError:
        pytest.skip("libcryptsetup.so.12 cannot be loaded")
    vp = ctypes.c_void_p
    L.crypt_init.argtypes = [ctypes.POINTER(vp), ctypes.c_char_p]
    L.crypt_format.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                               ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    L.crypt_volume_key_get.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
                                       ctypes.c_char_p, ctypes.c_size_t]
    L.crypt_free.argtypes = [vp]
    L.crypt_free.restype = None
    return L


@pytest.mark.parametrize("blocks", [1, 2, 127, 128, 129, 16385])
def test_oracle_equals_libcryptsetup(cryptsetup, tmp_path, blocks):
    L = cryptsetup
    data = np.random.default_rng(blocks).integers(0, 256, blocks * 512, dtype=np.uint8).tobytes()
    lay = vo.layout(len(data))
    tree, root = vo.tree(data)
    path = str(tmp_path / "image").encode()
    with open(path, "wb") as f:  # room for the tree: cryptsetup writes into the file, it does not grow it
        f.write(data + bytes(lay["hash_offset"] - len(data)) + b"\xEE" * max(lay["tree_bytes"], 4096))
    cd = ctypes.c_void_p()
    assert L.crypt_init(ctypes.byref(cd), path) == 0
    try:
        p = _VerityParams(hash_name=b"sha256", data_device=path, hash_type=1, data_block_size=512,
                          hash_block_size=4096, data_size=blocks, hash_area_offset=lay["hash_offset"],
                          flags=1 | 4)  # CRYPT_VERITY_NO_HEADER | CRYPT_VERITY_CREATE_HASH
        rc = L.crypt_format(cd, b"VERITY", None, None, None, None, 0, ctypes.byref(p))
        assert rc == 0, f"crypt_format(VERITY) on a plain file returned {rc}"
        key = ctypes.create_string_buffer(64)
        n = ctypes.c_size_t(64)
        assert L.crypt_volume_key_get(cd, -1, key, ctypes.byref(n), None, 0) == 0
    finally:
        L.crypt_free(cd)
    assert key.raw[:n.value] == root
    with open(path, "rb") as f:
        f.seek(lay["hash_offset"])
        assert f.read(lay["tree_bytes"]) == tree


def test_verity_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "verity_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "verity_plan_test.cpp"), "-o", exe])
    for seed in ("1", "2", "3"):
        out = subprocess.check_output([exe, seed], text=True, timeout=120)
        assert out.startswith("ok 20000"), out
