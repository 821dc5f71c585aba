"""Verity verify on the CPU: the hashlib restatement of the per-block verdicts
(tests/verity_verify_oracle.py) on clean and singly damaged images, pinned to
libcryptsetup's own userspace verification where that library can be loaded;
the stand-alone sanitizer program over csrc/verity_verify_plan.hpp
(tests/cpp/verity_verify_plan_test.cpp); parse_verity_label; the new symbols
of libnydusgpu.so.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nydus_gpu
import verity_oracle as vo
import verity_verify_oracle as vvo

from conftest import ROOT

SHAPES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 16383, 16384, 16385, 16514, 32769]


@pytest.fixture(scope="module")
def image():
    """(max(SHAPES) blocks of data, their leaf digests): every shape is a
    prefix, so the data is hashed once."""
    data = np.random.default_rng(0x5CA9).integers(0, 256, max(SHAPES) * 512, dtype=np.uint8).tobytes()
    return data, vo.leaf_digests(data)


@pytest.mark.parametrize("blocks", SHAPES)
def test_clean_images_have_no_findings(image, blocks):
    data, dig = image
    tree, root = vo.tree_from_leaves(dig[:blocks])
    assert vvo.verdicts_from_leaves(dig[:blocks], tree, root) == ([], [], [])
    assert vvo.findings(([], [], []), blocks, vo.layout(blocks * 512)["hash_offset"]) == []
    if blocks <= 257:
        assert vvo.verdicts(data[:blocks * 512], tree, root) == ([], [], [])


@pytest.mark.parametrize("blocks,kind", [(b, k) for b in (1, 2, 128, 129, 16385, 16514) for k in vvo.KINDS
                                         if vvo.applies(k, b)])
def test_single_damage_gives_exactly_its_findings(image, blocks, kind):
    data, dig = image
    tree, root = vo.tree_from_leaves(dig[:blocks])
    d, t, r, want = vvo.damage(kind, data[:blocks * 512], tree, root)
    assert any(want), kind
    assert vvo.verdicts(d, t, r) == want
    # the rebuild-and-compare view of the same thing: not clean either
    assert vo.tree(d) != (t, r)


def test_findings_order_and_ranges():
    # 16514 blocks: levels of 130 / 2 / 1 hash blocks at tree blocks 3 / 1 / 0
    lay = vo.layout(16514 * 512)
    assert (lay["level_blocks"], lay["first"]) == ([130, 2, 1], [3, 1, 0])
    got = vvo.findings(([5, 16513], [132, 0, 2], [0, 1]), 16514, 1 << 24)
    assert [(f["reason"], f["level"], f["block"]) for f in got] == \
        [("HASH", 2, 0), ("HASH", 1, 2), ("SPARE", 1, 2), ("HASH", 0, 132), ("SPARE", 0, 132),
         ("DATA", 0, 5), ("DATA", 0, 16513)]
    assert [(f["first_data_block"], f["last_data_block"]) for f in got] == \
        [(0, 16513), (16384, 16513), (16384, 16513), (16512, 16513), (16512, 16513), (5, 5), (16513, 16513)]
    assert [f["file_offset"] for f in got] == [1 << 24, (1 << 24) + 8192, (1 << 24) + 8192,
                                               (1 << 24) + 132 * 4096, (1 << 24) + 132 * 4096,
                                               5 * 512, 16513 * 512]


# ---- the pin to libcryptsetup --------------------------------------------------------
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
    L.crypt_activate_by_volume_key.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                               ctypes.c_uint32]
    L.crypt_set_log_callback.argtypes = [vp, ctypes.c_void_p, vp]
    L.crypt_set_log_callback.restype = None
    L.crypt_free.argtypes = [vp]
    L.crypt_free.restype = None
    return L


def _cryptsetup_verify(L, path, data, tree, root) -> int:
    """libcryptsetup's userspace check of the stored tree (CRYPT_VERITY_NO_HEADER |
    CRYPT_VERITY_CHECK_HASH, no CREATE_HASH; crypt_load would want a superblock)
    on a plain file holding data, gap and tree."""
    blocks = len(data) // 512
    off = vo.layout(len(data))["hash_offset"]
    with open(path, "wb") as f:  # one data block: no tree, but the hash area must exist
        f.write(data + bytes(off - len(data)) + (tree if tree else bytes(4096)))
    cd = ctypes.c_void_p()
    assert L.crypt_init(ctypes.byref(cd), path) == 0
    try:
        p = _VerityParams(hash_name=b"sha256", data_device=path, hash_type=1, data_block_size=512,
                          hash_block_size=4096, data_size=blocks, hash_area_offset=off, flags=1 | 2)
        rc = L.crypt_format(cd, b"VERITY", None, None, None, None, 0, ctypes.byref(p))
        assert rc == 0, f"crypt_format(VERITY) on a plain file returned {rc}"
        return L.crypt_activate_by_volume_key(cd, None, root, 32, 0)
    finally:
        L.crypt_free(cd)


@pytest.mark.parametrize("blocks", [1, 2, 128, 129, 16385])
def test_no_findings_iff_libcryptsetup_verifies(cryptsetup, image, tmp_path, blocks):
    data, dig = image
    data = data[:blocks * 512]
    tree, root = vo.tree_from_leaves(dig[:blocks])
    path = str(tmp_path / "image").encode()
    assert _cryptsetup_verify(cryptsetup, path, data, tree, root) == 0
    assert vvo.verdicts(data, tree, root) == ([], [], [])
    ran = []
    for kind in vvo.KINDS:
        if not vvo.applies(kind, blocks):
            continue
        d, t, r, want = vvo.damage(kind, data, tree, root)
        rc = _cryptsetup_verify(cryptsetup, path, d, t, r)
        found = vvo.verdicts(d, t, r)
        assert found == want and any(found), kind
        assert rc != 0, f"libcryptsetup accepts the '{kind}' damage the oracle finds {found}"
        ran.append(kind)
    # a hash-consistent tree with a non-zero spare byte is refused too ("Spare
    # area is not zeroed"): that is why the spare area is a finding of its own
    assert ("spare_consistent" in ran) == (blocks % 128 != 0 and blocks > 1)


# ---- the geometry header, the label, the library -----------------------------------------
def test_verity_verify_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "verity_verify_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "verity_verify_plan_test.cpp"), "-o", exe])
    for seed in ("1", "2", "3"):
        out = subprocess.check_output([exe, seed], text=True, timeout=300)
        assert out.startswith("ok 20000"), out


def test_parse_verity_label_is_the_inverse_of_verity_label():
    root = bytes(range(32)).hex()
    for n, off in ((1, 4096), (129, 69632), (379918, 194519040), ((1 << 53) - 1, 1 << 62)):
        info = {"data_blocks": n, "hash_offset": off, "root": root}
        assert nydus_gpu.parse_verity_label(nydus_gpu.verity_label(info)) == info
    assert nydus_gpu.parse_verity_label(f" 2,4096,sha256:{root.upper()}\n")["root"] == root
    for bad in ("", "1,4096", f"1,4096,{root}", f"1,4096,sha512:{root}", f"1,4096,sha256:{root[:-2]}",
                f"1,4096,sha256:{root[:-1]}g", f"x,4096,sha256:{root}", f"1,-4096,sha256:{root}",
                f"1,4096,sha256:{root},7"):
        with pytest.raises(ValueError):
            nydus_gpu.parse_verity_label(bad)


def test_library_exports_the_verify_calls():
    L = nydus_gpu.lib()
    for name in ("ngpu_verity_verify_tree_device", "ngpu_verity_verify_data_device",
                 "ngpu_verity_verify_image"):
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    assert nydus_gpu.VERITY_BAD_DTYPE.itemsize == 40 and ctypes.sizeof(nydus_gpu._lib.NgpuVerityReport) == 64
    # argument checks that need no GPU
    assert L.ngpu_verity_verify_image(None, nydus_gpu._lib.READ_AT_FN(), None, 512, 4096, bytes(32), None,
                                      None, None, 0) == nydus_gpu.EINVAL
