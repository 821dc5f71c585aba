"""Dict retire's C ABI without a GPU: the three symbols exist (additive in ABI
7), the info struct keeps its size, and the argument rejections that come before
any device work -- a NULL base, flags != 0, a count without a list, no out --
answer NGPU_EINVAL and clear *out."""
import ctypes

import nydus_gpu

SYMBOLS = ("ngpu_dict_retire", "ngpu_node_dict_retire", "ngpu_dict_export")


def test_library_exports_dict_retire():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    info = nydus_gpu._lib.NgpuDictInfo
    assert ctypes.sizeof(info) == 48 and info.has_blob_table.offset == 36  # a reserved word until now
    for m in ("retire", "export"):
        assert callable(getattr(nydus_gpu.ChunkDict, m))
    assert callable(nydus_gpu.Node.dict_retire) and callable(nydus_gpu.Node.dict_export)


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    # stand-ins for handles: the calls below must answer before looking at them
    eng = ctypes.create_string_buffer(4096)
    base = ctypes.create_string_buffer(4096)
    idx = (ctypes.c_uint32 * 2)(0, 1)
    e, b, i = (ctypes.cast(x, ctypes.c_void_p) for x in (eng, base, idx))
    for fn in (L.ngpu_dict_retire, L.ngpu_node_dict_retire):
        for args in ((e, None, i, 2, 0),            # NULL base
                     (e, b, i, 2, 1),               # flags != 0
                     (e, b, i, 2, 0x80000000),
                     (e, b, None, 2, 0),            # n without blobs
                     (None, b, i, 2, 0),            # no engine / node
                     (None, None, None, 0, 0)):
            out = ctypes.c_void_p(0xDEAD)
            assert fn(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, (fn.__name__, args[3:])
            assert out.value is None
        assert fn(e, b, i, 2, 0, None) == nydus_gpu.EINVAL  # no out
        assert fn(e, None, i, 2, 0, None) == nydus_gpu.EINVAL
    # export: the counts are always set, to 0 without a dict
    m, nb = ctypes.c_uint64(7), ctypes.c_uint32(7)
    assert L.ngpu_dict_export(e, None, None, 0, ctypes.byref(m), None, 0, ctypes.byref(nb)) == nydus_gpu.EINVAL
    assert (m.value, nb.value) == (0, 0)
    assert L.ngpu_dict_export(None, None, None, 0, None, None, 0, None) == nydus_gpu.EINVAL
