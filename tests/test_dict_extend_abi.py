"""Dict extend's C ABI without a GPU: the four symbols exist (additive in ABI
7), the info struct has the header's layout, and the argument rejections that
come before any device work -- a NULL base, flags != 0, records missing --
answer NGPU_EINVAL and clear *out."""
import ctypes

import nydus_gpu

SYMBOLS = ("ngpu_dict_extend", "ngpu_dict_extend_bootstrap", "ngpu_node_dict_extend",
           "ngpu_dict_info_get")


def test_library_exports_dict_extend():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    assert ctypes.sizeof(nydus_gpu._lib.NgpuDictInfo) == 48
    for m in ("extend", "extend_bootstrap", "info"):
        assert callable(getattr(nydus_gpu.ChunkDict, m))
    assert callable(nydus_gpu.Node.dict_extend)


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    # stand-ins for handles: the calls below must answer before looking at them
    eng = ctypes.create_string_buffer(4096)
    base = ctypes.create_string_buffer(4096)
    recs = ctypes.create_string_buffer(80)
    e, b, r = (ctypes.cast(x, ctypes.c_void_p) for x in (eng, base, recs))
    for fn in (L.ngpu_dict_extend, L.ngpu_node_dict_extend):
        for args in ((e, None, r, 1, None, 0, 0),     # NULL base
                     (e, b, r, 1, None, 0, 1),        # flags != 0
                     (e, b, r, 1, None, 0, 0x80000000),
                     (None, None, None, 0, None, 0, 0)):
            out = ctypes.c_void_p(0xDEAD)
            assert fn(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, (fn.__name__, args[3:])
            assert out.value is None
        assert fn(e, None, r, 1, None, 0, 0, None) == nydus_gpu.EINVAL  # no out either
    for args in ((e, None, b"/nonexistent", 0), (e, b, b"/nonexistent", 2), (e, None, None, 0)):
        out = ctypes.c_void_p(0xDEAD)
        assert L.ngpu_dict_extend_bootstrap(*args, ctypes.byref(out)) == nydus_gpu.EINVAL
        assert out.value is None
    info = nydus_gpu._lib.NgpuDictInfo()
    assert L.ngpu_dict_info_get(None, ctypes.byref(info)) == nydus_gpu.EINVAL
    assert L.ngpu_dict_info_get(b, None) == nydus_gpu.EINVAL
