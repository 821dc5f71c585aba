"""The C ABI of node dict retire / export across parts without a GPU: the two
symbols exist (additive in ABI 7), the Python view has them, and the argument
rejections that come before any handle is looked at -- a NULL node, base or out,
flags != 0, a count without a list, an export without a dict -- answer
NGPU_EINVAL, clear *out and zero the export's counts."""
import ctypes

import nydus_gpu

SYMBOLS = ("ngpu_node_dict_retire_parts", "ngpu_node_dict_export")


def test_library_exports_node_dict_retire_parts():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    assert callable(nydus_gpu.Node.dict_retire_parts) and callable(nydus_gpu.Node.dict_export_parts)
    # the calls they stand next to are still there
    assert callable(nydus_gpu.Node.dict_retire) and callable(nydus_gpu.Node.dict_export)


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    # stand-ins for handles: the calls below must answer before looking at them
    node = ctypes.create_string_buffer(4096)
    base = ctypes.create_string_buffer(4096)
    idx = (ctypes.c_uint32 * 2)(0, 1)
    nd, b, i = (ctypes.cast(x, ctypes.c_void_p) for x in (node, base, idx))
    fn = L.ngpu_node_dict_retire_parts
    for args in ((nd, None, i, 2, 0),            # NULL base
                 (nd, b, i, 2, 1),               # flags != 0
                 (nd, b, i, 2, 0x80000000),
                 (nd, b, None, 2, 0),            # n without blobs
                 (None, b, i, 2, 0),             # no node
                 (None, None, None, 0, 0)):
        out = ctypes.c_void_p(0xDEAD)
        assert fn(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, args[3:]
        assert out.value is None
    assert fn(nd, b, i, 2, 0, None) == nydus_gpu.EINVAL  # no out
    assert fn(nd, None, i, 2, 0, None) == nydus_gpu.EINVAL
    # export: the counts are always set, to 0 without a dict
    ex = L.ngpu_node_dict_export
    m, nb = ctypes.c_uint64(7), ctypes.c_uint32(7)
    assert ex(nd, None, None, 0, ctypes.byref(m), None, 0, ctypes.byref(nb), 0) == nydus_gpu.EINVAL
    assert (m.value, nb.value) == (0, 0)
    m.value = nb.value = 7
    assert ex(None, None, None, 0, ctypes.byref(m), None, 0, ctypes.byref(nb), 0) == nydus_gpu.EINVAL
    assert (m.value, nb.value) == (0, 0)
    assert ex(None, None, None, 0, None, None, 0, None, 0) == nydus_gpu.EINVAL
    # flags != 0 and a missing node, with a (zeroed) dict: the counts are the dict's, 0 here
    for args in ((nd, b, 1), (nd, b, 0x80000000), (None, b, 0)):
        m.value = nb.value = 7
        assert ex(args[0], args[1], None, 0, ctypes.byref(m), None, 0, ctypes.byref(nb), args[2]) == nydus_gpu.EINVAL
        assert (m.value, nb.value) == (0, 0)
    assert ex(nd, b, None, 0, None, None, 0, ctypes.byref(nb), 0) == nydus_gpu.EINVAL  # no n_records
    assert ex(nd, b, None, 0, ctypes.byref(m), None, 0, None, 0) == nydus_gpu.EINVAL   # no n_blobs
