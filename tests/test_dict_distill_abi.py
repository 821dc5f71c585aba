"""Dict distill's C ABI without a GPU: the two symbols exist (additive in ABI 7),
the info struct has its size, and the argument rejections that come before any
device work -- a NULL base, engine or node, flag bits other than the two, both
flags together -- answer NGPU_EINVAL, clear *out and zero info.  (No out and no
info is a valid count-only call shape: it is not among the refusals.)"""
import ctypes

import nydus_gpu

SYMBOLS = ("ngpu_dict_distill", "ngpu_node_dict_distill")
KEEP, MERGE = 0x1, 0x2  # NGPU_DICT_DISTILL_KEEP_BLOBS, NGPU_DICT_DISTILL_MERGE_BLOB_IDS


def test_library_exports_dict_distill():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    info = nydus_gpu.NgpuDictDistillInfo
    assert ctypes.sizeof(info) == 312
    assert (info.entries_out.offset, info.blobs_in.offset, info.max_refs.offset, info.refs_hist.offset) == \
        (32, 40, 48, 56)
    assert (nydus_gpu.DICT_DISTILL_KEEP_BLOBS, nydus_gpu.DICT_DISTILL_MERGE_BLOB_IDS) == (KEEP, MERGE)
    x = info()
    x.max_refs, x.refs_hist[31] = 7, 9
    d = x.as_dict()
    assert d["max_refs"] == 7 and d["refs_hist"][31] == 9 and len(d["refs_hist"]) == 32 and "reserved" not in d
    assert callable(nydus_gpu.ChunkDict.distill) and callable(nydus_gpu.Node.dict_distill)


def test_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    # stand-ins for handles: the calls below must answer before looking at them
    eng = ctypes.create_string_buffer(4096)
    base = ctypes.create_string_buffer(4096)
    e, b = (ctypes.cast(x, ctypes.c_void_p) for x in (eng, base))
    for fn in (L.ngpu_dict_distill, L.ngpu_node_dict_distill):
        for args in ((e, None, 1, 0),               # NULL base
                     (None, b, 1, 0),               # no engine / node
                     (None, None, 0, 0),
                     (e, b, 1, 4),                  # unknown flag bits
                     (e, b, 1, 0x80000000),
                     (e, b, 1, KEEP | 8),
                     (e, b, 1, KEEP | MERGE),       # nothing is merged with KEEP_BLOBS: refused
                     (e, b, 0xFFFFFFFF, KEEP | MERGE)):
            out = ctypes.c_void_p(0xDEAD)
            info = nydus_gpu.NgpuDictDistillInfo()
            ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
            assert fn(*args, ctypes.byref(out), ctypes.byref(info)) == nydus_gpu.EINVAL, (fn.__name__, args[2:])
            assert out.value is None
            assert bytes(info) == bytes(312), (fn.__name__, args[2:])
            # each of the two may be left out
            assert fn(*args, None, ctypes.byref(info)) == nydus_gpu.EINVAL
            out = ctypes.c_void_p(0xDEAD)
            assert fn(*args, ctypes.byref(out), None) == nydus_gpu.EINVAL and out.value is None
            assert fn(*args, None, None) == nydus_gpu.EINVAL
