"""The C ABI of node dict distill across parts without a GPU: the symbol exists
(additive in ABI 7), the Python view has it, and the argument rejections that come
before any handle is looked at -- a NULL node, a NULL base, a flag bit other than
the two, both flags together -- answer NGPU_EINVAL, clear *out and zero info's 312
bytes, with and without an out."""
import ctypes

import nydus_gpu
from nydus_gpu import _lib

SYMBOL = "ngpu_node_dict_distill_parts"
BOTH = nydus_gpu.DICT_DISTILL_KEEP_BLOBS | nydus_gpu.DICT_DISTILL_MERGE_BLOB_IDS


def test_library_exports_node_dict_distill_parts():
    L = nydus_gpu.lib()
    assert SYMBOL in nydus_gpu.EXPORTS and hasattr(L, SYMBOL)
    assert L.ngpu_abi_version() == 7
    assert callable(nydus_gpu.Node.dict_distill_parts)
    # the call it stands next to is still there
    assert callable(nydus_gpu.Node.dict_distill) and "ngpu_node_dict_distill" in nydus_gpu.EXPORTS


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    assert ctypes.sizeof(_lib.NgpuDictDistillInfo) == 312
    # stand-ins for handles: the calls below must answer before looking at them
    node = ctypes.create_string_buffer(4096)
    base = ctypes.create_string_buffer(4096)
    nd, b = (ctypes.cast(x, ctypes.c_void_p) for x in (node, base))
    fn = getattr(L, SYMBOL)
    for args in ((None, b, 1, 0),       # NULL node
                 (nd, None, 1, 0),      # NULL base
                 (None, None, 0, 0),
                 (nd, b, 1, 0x4),       # a flag bit other than the two
                 (nd, b, 1, 0x80000000),
                 (nd, b, 1, BOTH),      # both flags together
                 (nd, b, 0, BOTH | 0x4)):
        for with_out in (True, False):
            out = ctypes.c_void_p(0xDEAD)
            info = _lib.NgpuDictDistillInfo()
            ctypes.memset(ctypes.byref(info), 0xA5, 312)
            rc = fn(*args, ctypes.byref(out) if with_out else None, ctypes.byref(info))
            assert rc == nydus_gpu.EINVAL, (args[2:], with_out)
            if with_out:
                assert out.value is None
            assert bytes(info) == bytes(312), (args[2:], with_out)
        # and with no info either
        out = ctypes.c_void_p(0xDEAD)
        assert fn(*args, ctypes.byref(out), None) == nydus_gpu.EINVAL
        assert out.value is None
        assert fn(*args, None, None) == nydus_gpu.EINVAL
