"""The C ABI of dict save without a GPU: the three symbols exist (additive in ABI
7), the Python view has them, the two structs are 40 and 64 bytes,
ngpu_dict_save_layout gives the layout rafs.write_v6_bootstrap writes and
rafs.read_v6 reads back, and the argument rejections that come before any handle is
looked at -- a NULL engine, node, dict or writer -- answer NGPU_EINVAL and zero
*info."""
import ctypes

import numpy as np
import pytest

import nydus_gpu
from nydus_gpu import _lib, rafs

SYMBOLS = ("ngpu_dict_save_layout", "ngpu_dict_save", "ngpu_node_dict_save")


def test_library_exports_dict_save():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    assert callable(nydus_gpu.ChunkDict.save) and callable(nydus_gpu.Node.dict_save)
    assert callable(nydus_gpu.dict_save_layout) and nydus_gpu.DICT_SAVE_NO_BLOB_TABLE == 0x1
    # the calls it stands next to are still there
    assert callable(nydus_gpu.ChunkDict.export) and callable(nydus_gpu.Node.dict_export_parts)


def test_struct_sizes():
    assert ctypes.sizeof(_lib.NgpuDictSaveOptions) == 40
    assert ctypes.sizeof(_lib.NgpuDictSaveInfo) == 64
    assert _lib.NgpuDictSaveOptions.window_records.offset == 16
    assert _lib.NgpuDictSaveOptions.reserved.offset == 24
    assert _lib.NgpuDictSaveInfo.windows.offset == 56


@pytest.mark.parametrize("b", [0, 1, 15, 16, 17, 33])
@pytest.mark.parametrize("k", [0, 1, 51, 52, 4097])
def test_layout_is_the_python_writer_s(k, b):
    cs = 0x10000
    boot = rafs.write_v6_bootstrap(np.zeros(k, rafs.CHUNK_INFO_DTYPE), cs, blobs=np.zeros(b, rafs.BLOB_DTYPE))
    lay = nydus_gpu.dict_save_layout(k, b)
    assert lay["bytes"] == len(boot)
    back = rafs.read_v6(boot)
    for f in ("blob_table_offset", "blob_table_size", "chunk_table_offset", "chunk_table_size"):
        assert lay[f] == back[f], f
    assert (lay["entries"], lay["blobs"], lay["windows"]) == (k, b, 0)


def test_layout_edges_and_limits():
    lay = nydus_gpu.dict_save_layout(0xFFFFFFFE, 1 << 20)
    assert lay["chunk_table_offset"] == 4096 + (256 << 20)
    assert lay["bytes"] == lay["chunk_table_offset"] + 80 * 0xFFFFFFFE
    assert nydus_gpu.dict_save_layout(5, 16)["chunk_table_offset"] == 8192
    assert nydus_gpu.dict_save_layout(5, 17)["chunk_table_offset"] == 12288
    L = nydus_gpu.lib()
    for k, b in ((0xFFFFFFFF, 0), (1 << 40, 1), (1, (1 << 20) + 1)):
        x = _lib.NgpuDictSaveInfo(bytes=7, entries=7)
        assert L.ngpu_dict_save_layout(k, b, ctypes.byref(x)) == nydus_gpu.EINVAL
        assert (x.bytes, x.entries) == (0, 0)
        with pytest.raises(nydus_gpu.NgpuError):
            nydus_gpu.dict_save_layout(k, b)
    assert L.ngpu_dict_save_layout(1, 1, None) == nydus_gpu.EINVAL


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    # stand-ins for handles: the calls below must answer before looking at them
    eng = ctypes.create_string_buffer(4096)
    dct = ctypes.create_string_buffer(4096)
    e, d = (ctypes.cast(x, ctypes.c_void_p) for x in (eng, dct))
    calls = []
    fn = _lib.WRITE_FN(lambda _c, _b, n: calls.append(n) or 0)
    null_fn = _lib.WRITE_FN()
    opt = _lib.NgpuDictSaveOptions()
    for save in (L.ngpu_dict_save, L.ngpu_node_dict_save):
        for args in ((None, d, fn), (e, None, fn), (e, d, null_fn), (None, None, null_fn)):
            info = _lib.NgpuDictSaveInfo(entries=7, bytes=7, windows=7)
            assert save(args[0], args[1], ctypes.byref(opt), args[2], None, ctypes.byref(info)) == nydus_gpu.EINVAL
            assert (info.entries, info.bytes, info.windows) == (0, 0, 0)
            assert save(args[0], args[1], None, args[2], None, None) == nydus_gpu.EINVAL  # no info, no options
    assert calls == []
