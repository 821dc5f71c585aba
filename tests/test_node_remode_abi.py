"""The C ABI of node dict remode without a GPU: the two symbols exist (additive in
ABI 7), the Python view has them, the two structures have their sizes, and the
argument rejections that come before any handle is looked at -- a NULL node, base
or out, non-zero option flags or reserved word -- answer NGPU_EINVAL and clear
*out; ngpu_node_dict_info_get with a NULL argument zeroes its 528 bytes."""
import ctypes

import nydus_gpu
from nydus_gpu import _lib

SYMBOLS = ("ngpu_node_dict_remode", "ngpu_node_dict_info_get")


def test_library_exports_node_dict_remode():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    assert callable(nydus_gpu.Node.dict_remode) and callable(nydus_gpu.Node.dict_info)
    assert ctypes.sizeof(_lib.NgpuNodeDictRemodeOptions) == 16
    assert ctypes.sizeof(_lib.NgpuNodeDictInfo) == 528
    # the calls they stand next to are still there
    assert callable(nydus_gpu.Node.dict_create) and callable(nydus_gpu.Node.dict_export_parts)


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    Opt = _lib.NgpuNodeDictRemodeOptions
    # stand-ins for handles: the calls below must answer before looking at them
    node = ctypes.create_string_buffer(4096)
    base = ctypes.create_string_buffer(4096)
    nd, b = (ctypes.cast(x, ctypes.c_void_p) for x in (node, base))
    fn = L.ngpu_node_dict_remode
    zeros, windowed = Opt(0, 0, 0), Opt(0, 0, 100)
    for mode in (nydus_gpu.NODE_DICT_PARTITION, nydus_gpu.NODE_DICT_REPLICATE,
                 nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_ROUTED):
        for args in ((None, b, mode, None),                 # NULL node
                     (nd, None, mode, None),                # NULL base
                     (None, None, mode, ctypes.byref(zeros)),
                     (None, b, mode, ctypes.byref(windowed)),
                     (nd, b, mode, ctypes.byref(Opt(1, 0, 0))),           # flags
                     (nd, b, mode, ctypes.byref(Opt(0x80000000, 0, 0))),
                     (nd, b, mode, ctypes.byref(Opt(0, 1, 0))),           # reserved
                     (nd, b, mode, ctypes.byref(Opt(0, 0x80000000, 64))),
                     (nd, b, mode, ctypes.byref(Opt(1, 1, 0)))):
            out = ctypes.c_void_p(0xDEAD)
            assert fn(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, (mode, args[3])
            assert out.value is None
        assert fn(nd, b, mode, None, None) == nydus_gpu.EINVAL  # NULL out
        assert fn(nd, b, mode, ctypes.byref(zeros), None) == nydus_gpu.EINVAL
        assert fn(None, None, mode, None, None) == nydus_gpu.EINVAL


def test_info_get_with_a_null_argument_zeroes_its_bytes():
    L = nydus_gpu.lib()
    node = ctypes.create_string_buffer(4096)
    d = ctypes.create_string_buffer(4096)
    nd, dd = (ctypes.cast(x, ctypes.c_void_p) for x in (node, d))
    fn = L.ngpu_node_dict_info_get
    for args in ((None, dd), (nd, None), (None, None)):
        info = _lib.NgpuNodeDictInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, 528)
        assert fn(*args, ctypes.byref(info)) == nydus_gpu.EINVAL
        assert bytes(info) == bytes(528), args
    assert fn(nd, dd, None) == nydus_gpu.EINVAL  # nowhere to write
    assert fn(None, None, None) == nydus_gpu.EINVAL
