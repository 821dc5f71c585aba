"""Node dict fold's C ABI without a GPU: the symbol exists (additive in ABI 7),
ngpu_node_fold_part is 40 bytes, and the argument rejections that come before any
device work -- a NULL node, base, parts or out, flags != 0, a count without its
array -- answer NGPU_EINVAL and clear *out."""
import ctypes
import os
import re

import nydus_gpu
from conftest import ROOT


def test_library_exports_node_dict_fold():
    L = nydus_gpu.lib()
    assert "ngpu_node_dict_fold" in nydus_gpu.EXPORTS and hasattr(L, "ngpu_node_dict_fold")
    assert L.ngpu_abi_version() == 7
    assert callable(nydus_gpu.Node.dict_fold)


def test_fold_part_is_40_bytes_as_the_header_says():
    from nydus_gpu import _lib
    P = _lib.NgpuNodeFoldPart
    assert ctypes.sizeof(P) == 40
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("d_results", 0), ("d_chunks", 8), ("n", 16), ("d_layer_first", 24), ("n_layers", 32)]
    with open(os.path.join(ROOT, "include", "nydus_gpu.h")) as f:
        h = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} ngpu_node_fold_part;", h).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in P._fields_]


def test_node_fold_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    # stand-ins for handles and tables: the calls below must answer before looking at them
    bufs = [ctypes.create_string_buffer(4096) for _ in range(5)]
    node, b, parts, pl, tbl = [(ctypes.addressof(x) + 63) & ~63 for x in bufs]
    #        node base parts np place n_place table nb flags
    cases = [(None, b, parts, 2, None, 0, None, 0, 0),          # NULL node
             (node, None, parts, 2, None, 0, None, 0, 0),       # NULL base
             (node, b, None, 2, None, 0, None, 0, 0),           # NULL parts
             (node, b, None, 0, None, 0, None, 0, 0),           # (whatever their count is)
             (node, b, parts, 2, None, 0, None, 0, 1),          # flags != 0
             (node, b, parts, 2, None, 0, None, 0, 0x80000000),
             (node, b, parts, 2, None, 3, None, 0, 0),          # a placement count without rows
             (node, b, parts, 2, pl, 3, None, 2, 0),            # a blob count without a table
             (None, None, None, 0, None, 0, None, 0, 0)]
    for args in cases:
        out = ctypes.c_void_p(0xDEAD)
        assert L.ngpu_node_dict_fold(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, args[3:]
        assert out.value is None
    assert L.ngpu_node_dict_fold(node, b, parts, 2, pl, 3, tbl, 2, 0, None) == nydus_gpu.EINVAL  # no out
    del bufs
