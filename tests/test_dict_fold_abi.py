"""Dict fold's C ABI without a GPU: the two symbols exist (additive in ABI 7),
ngpu_dict_place is 16 bytes, and the argument rejections that come before any
device work -- a NULL base or engine, flags != 0, counts without their arrays, a
misaligned result table, descriptor table, layer cuts or digest array, no out --
answer NGPU_EINVAL and clear *out."""
import ctypes

import numpy as np

import nydus_gpu

SYMBOLS = ("ngpu_dict_fold", "ngpu_dict_extend_device")


def test_library_exports_dict_fold():
    L = nydus_gpu.lib()
    for name in SYMBOLS:
        assert name in nydus_gpu.EXPORTS and hasattr(L, name), name
    assert L.ngpu_abi_version() == 7
    assert nydus_gpu.DICT_PLACE_DTYPE.itemsize == 16
    assert nydus_gpu.DICT_PLACE_DTYPE.names == ("compressed_offset", "compressed_size", "flags")
    assert [nydus_gpu.DICT_PLACE_DTYPE.fields[f][1] for f in nydus_gpu.DICT_PLACE_DTYPE.names] == [0, 8, 12]
    for m in ("fold", "extend_device"):
        assert callable(getattr(nydus_gpu.ChunkDict, m))


def _handles():
    # stand-ins for handles and tables: the calls below must answer before looking at them
    bufs = [ctypes.create_string_buffer(4096) for _ in range(4)]
    return bufs, [(ctypes.addressof(b) + 63) & ~63 for b in bufs]  # 64-byte aligned addresses inside


def test_fold_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    bufs, (e, b, r, c) = _handles()
    place = np.zeros(2, nydus_gpu.DICT_PLACE_DTYPE)
    p = place.ctypes.data
    #        eng base res  chunks n  first L  place np table nb flags
    cases = [(e, None, r, c, 4, None, 1, None, 0, None, 0, 0),           # NULL base
             (None, b, r, c, 4, None, 1, None, 0, None, 0, 0),           # no engine
             (e, b, r, c, 4, None, 1, None, 0, None, 0, 1),              # flags != 0
             (e, b, r, c, 4, None, 1, None, 0, None, 0, 0x80000000),
             (e, b, None, c, 4, None, 1, None, 0, None, 0, 0),           # n without results
             (e, b, r, None, 4, None, 1, None, 0, None, 0, 0),           # n without descriptors
             (e, b, r + 8, c, 4, None, 1, None, 0, None, 0, 0),          # results not 16-byte aligned
             (e, b, r + 4, c, 0, None, 1, None, 0, None, 0, 0),          # (whatever n is)
             (e, b, r, c + 4, 4, None, 1, None, 0, None, 0, 0),          # descriptors not 8-byte aligned
             (e, b, r, c, 4, c + 4, 2, None, 0, None, 0, 0),             # layer cuts not 8-byte aligned
             (e, b, r, c, 4, None, 1, None, 2, None, 0, 0),              # a placement count without rows
             (e, b, r, c, 4, None, 1, p, 2, None, 1, 0),                 # a blob count without a table
             (None, None, None, None, 0, None, 0, None, 0, None, 0, 0)]
    for args in cases:
        out = ctypes.c_void_p(0xDEAD)
        assert L.ngpu_dict_fold(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, args[4:]
        assert out.value is None
    assert L.ngpu_dict_fold(e, b, r, c, 4, None, 1, None, 0, None, 0, 0, None) == nydus_gpu.EINVAL  # no out
    del bufs


def test_extend_device_rejections_that_need_no_device():
    L = nydus_gpu.lib()
    bufs, (e, b, d, u) = _handles()
    #        eng base dg usize blob index uoff n nb flags
    cases = [(e, None, d, u, u, u, None, 4, 1, 0),        # NULL base
             (None, b, d, u, u, u, None, 4, 1, 0),        # no engine
             (e, b, d, u, u, u, None, 4, 1, 1),           # flags != 0
             (e, b, None, u, u, u, None, 4, 1, 0),        # n without digests
             (e, b, d, None, u, u, None, 4, 1, 0),        # n without sizes
             (e, b, d, u, None, u, None, 4, 1, 0),        # n without blob indices
             (e, b, d + 8, u, u, u, None, 4, 1, 0),       # digests not 16-byte aligned
             (None, None, None, None, None, None, None, 0, 0, 0)]
    for args in cases:
        out = ctypes.c_void_p(0xDEAD)
        assert L.ngpu_dict_extend_device(*args, ctypes.byref(out)) == nydus_gpu.EINVAL, args[7:]
        assert out.value is None
    assert L.ngpu_dict_extend_device(e, b, d, u, u, u, None, 4, 1, 0, None) == nydus_gpu.EINVAL  # no out
    del bufs
