"""Crafted-digest collision matrix on every dedup path (csrc/dedup.hip).

Every other dedup test hashes real bytes, and with real BLAKE3 / SHA-256
output the legs where the four hash-table implementations can go wrong never
run: an equal tag on an unequal digest, an equal digest at another length, the
0xFFFFFFFF -> 0xFFFFFFFE tag remap, long probe chains that wrap past the top of
the table, one slot every lane races on, prefixes past 2^32 in the small
kernels.  The cases of dedup_cases.py hold all of them; they enter through the
product ABI as records marked NGPU_DIGESTED (no byte is hashed) and must come
back byte-exact: every field of every chunk, every stats field, on

  lds256 / lds1024   dedup_small_lds<256> / <1024>   ngpu_dedup_device
  small              dedup_small                     ngpu_dedup_layers_device
                     (L = 1, and L = 3 with an empty middle layer), and
                     ngpu_dedup_device under a dict of 1,100 inner blobs
  grid               the six grid kernels            FLAG_GRID_STAGES, n > 4096

at fs v6 (4 KiB-aligned offsets) and v5, without a dict (a), with the engine
probing its dict (b), with hits from ngpu_dict_probe_device (c), and with some
of those hits edited to name a blob >= n_dict_blobs, which makes them misses.
The expectation is test_dedup_cases.model_dedup (equal to the oracle on every
case: test_dedup_cases.py, which also proves which kernel each call shape
selects); multi-layer calls expect the oracle on each layer's slice alone.
Single-layer outputs of one case are then compared across the paths.
"""
import hashlib

import numpy as np
import pytest

import dedup_cases as dc
import nydus_gpu
from test_dedup_cases import DICT, NONE, expect, model_dedup

pytestmark = pytest.mark.gpu

GRID = nydus_gpu.FLAG_GRID_STAGES
STAT_FIELDS = ("chunks", "new_chunks", "intra_chunks", "dict_chunks", "new_bytes",
               "uncompressed_size", "own_blob_index", "blobs")
_SEEN = {}  # (case, align, mode, layers) -> (path, sha256 of the records, stats): path against path


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _records(case):
    """What the digest stage leaves: the digest and the DIGESTED mark; every
    other field holds junk the dedup stage must overwrite."""
    rec = np.zeros(case.n, nydus_gpu.RESULT_DTYPE)
    rec["digest"] = case.digests
    rec["kind"] = nydus_gpu.DIGESTED
    rec["index"] = rec["blob_index"] = rec["dict_blob"] = 0xDEADBEEF
    rec["ref"] = rec["uncompressed_offset"] = 0xDEADBEEFDEADBEEF
    return rec


def _chunks(case):
    ch = np.zeros(case.n, nydus_gpu.CHUNK_DTYPE)
    ch["length"] = case.lengths
    ch["file_index"] = np.arange(case.n)
    return ch


def _layers_expectation(case, first, unusable, oracle):
    """Each layer's slice on its own (the oracle; the model where rows are
    unusable): NEW / INTRA refs are chunk ids of the call."""
    dd, ds, db, di, _, _ = case.dict
    dec, stats = [], []
    for a, b in zip(first[:-1], first[1:]):
        a, b = int(a), int(b)
        dg, ln = case.digests[a:b], case.lengths[a:b]
        if unusable is None and b > a:
            if case.m:
                e, own = oracle.dedup(dg, ln, dd, ds, db, di, case.align)
            else:
                e, own = oracle.dedup(dg, ln, align=case.align)
            m, st = model_dedup(dg, ln, dd, ds, db, di, None, case.align)
            assert (NONE if own is None else own) == st["own_blob_index"]
            for f in ("kind", "ref", "index", "blob_index", "uncompressed_offset"):
                assert np.array_equal(e[f], m[f]), f
            e = m
        else:
            e, st = model_dedup(dg, ln, dd, ds, db, di, None, case.align, unusable)
        e["ref"][e["kind"] != DICT] += a
        dec.append(e)
        stats.append(st)
    return np.concatenate(dec), stats


def _compare(tag, case, got, stats, exp, exp_stats):
    assert np.array_equal(got["digest"], case.digests), f"{tag}: digest changed"
    for f in ("kind", "ref", "index", "blob_index", "uncompressed_offset"):
        bad = np.flatnonzero(got[f] != exp[f])
        if len(bad):
            c = int(bad[0])
            cls = [k for k, gs in case.classes.items() if any(c in g for g in gs)]
            raise AssertionError(f"{tag}: {f} differs on {len(bad)} chunks, first chunk {c} "
                                 f"(classes {cls}): got {got[f][c]}, expected {exp[f][c]}")
    hit = got["kind"] == DICT
    assert np.array_equal(got["dict_blob"][hit], case.dict[2][exp["ref"][hit].astype(np.int64)]), tag
    assert (got["dict_blob"][~hit] == 0).all(), tag
    for l, (st, est) in enumerate(zip(stats, exp_stats)):
        for f in STAT_FIELDS:
            assert int(st[f]) == est[f], f"{tag}: layer {l} stats {f}: got {st[f]}, expected {est[f]}"


def _run(eng, path, case, mode, shapes, d_hits, n_blobs, unusable, oracle):
    """One dedup call per shape over fresh records.  shape None: one layer
    through ngpu_dedup_device; else the layer_first array of
    ngpu_dedup_layers_device."""
    import torch
    d_ch = _dev(_chunks(case))
    hp = d_hits.data_ptr() if d_hits is not None else 0
    for shape in shapes:
        out = _dev(_records(case))
        tag = f"{path} {case.name} align {case.align} mode {mode} " + \
              ("one layer" if shape is None else f"layer_first {list(shape)}")
        if shape is None:
            st = eng.dedup_device(d_ch.data_ptr(), case.n, out.data_ptr(), hp, n_blobs, want_stats=True)
            stats = [st]
            exp, est = expect(case, unusable, uoff=False)
            exp_stats = [est]
        else:
            L = len(shape) - 1
            d_first = torch.from_numpy(np.asarray(shape, np.int64)).cuda()
            d_st = torch.zeros(L * nydus_gpu.LAYER_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            eng.dedup_layers_device(d_ch.data_ptr(), case.n, out.data_ptr(), d_first.data_ptr(), L,
                                    d_st.data_ptr(), hp, n_blobs)
            torch.cuda.synchronize()
            stats = list(d_st.cpu().numpy().view(nydus_gpu.LAYER_STATS_DTYPE))
            exp, exp_stats = _layers_expectation(case, shape, unusable, oracle)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
        _compare(tag, case, got, stats, exp, exp_stats)
        eng.device_status()
        # the same case on another path: the same bytes, whatever the oracle says
        layers = 1 if shape is None else len(shape) - 1
        key = (case.name, case.align, mode, layers)
        mine = (path, hashlib.sha256(got.tobytes()).digest(), [tuple(int(s[f]) for f in STAT_FIELDS) for s in stats])
        other = _SEEN.setdefault(key, mine)
        assert other[1:] == mine[1:], f"{tag}: differs from path {other[0]}"


def _matrix(path, kind, n, flags, shapes, oracle, many=False):
    import torch
    for align, fs in ((4096, 6), (1, 5)):
        eng = nydus_gpu.Engine(chunk_size=dc.CHUNK_SIZE, fs_version=fs, flags=flags)
        try:
            if kind != "all_dict" and not many:  # (a) no dict
                _run(eng, path, dc.get(kind, n, align), "a", shapes, None, 0, None, oracle)
            if kind in ("hot", "distinct"):
                continue
            case = dc.get(kind, n, align, True, many)
            if not case.m:  # n = 1, 2: no room for a dict class
                continue
            dd, ds, db, di, _, n_blobs = case.dict
            keep = [_dev(x) for x in (dd, ds, db, di)]  # alive until the engine has copied them
            torch.cuda.synchronize()
            eng.dict_load_device(*(t.data_ptr() for t in keep), case.m, n_blobs)
            torch.cuda.synchronize()
            _run(eng, path, case, "b", shapes, None, 0, None, oracle)  # (b) the kernel probes
            rec = _dev(_records(case))
            hits = torch.empty((case.n, 6), dtype=torch.int32, device="cuda")  # ngpu_dict_hit, 24 B
            eng.dict_probe_device(rec.data_ptr(), 64, case.n, hits.data_ptr())
            torch.cuda.synchronize()
            _run(eng, path, case, "c", shapes, hits, n_blobs, None, oracle)  # (c) hits given
            # (c) again with every hit on three rows naming a blob >= n_dict_blobs: misses
            h = hits.cpu().numpy().view(np.uint32)
            ents = list(dict.fromkeys(int(e) for e in h[:, 0] if e != nydus_gpu.MISS))
            assert len(ents) >= 3
            rows = (ents[0], ents[len(ents) // 2], ents[-1])
            for r, bogus in zip(rows, (n_blobs, n_blobs + 7, 0xFFFFFFFE)):
                sel = torch.from_numpy(h[:, 0] == r).cuda()
                hits[sel, 2] = int(np.uint32(bogus).astype(np.int32))
            torch.cuda.synchronize()
            _run(eng, path, case, "c-edited", shapes, hits, n_blobs, lambda e: e in rows, oracle)
        finally:
            eng.close()


def _three(n):
    """L = 3: cuts at n / 3, the middle layer empty."""
    return [0, n // 3, n // 3, n]


PARAMS = [("lds256", n) for n in dc.PATH_N["lds256"]] + [("lds1024", n) for n in dc.PATH_N["lds1024"]] + \
         [("small", n) for n in dc.PATH_N["small"]] + [("grid", n) for n in dc.PATH_N["grid"]]


@pytest.mark.parametrize("path,n", PARAMS, ids=[f"{p}-{n}" for p, n in PARAMS])
def test_collision_matrix(path, n, oracle):
    if path in ("lds256", "lds1024"):
        _matrix(path, "mixed", n, 0, [None], oracle)
    elif path == "small":
        _matrix(path, "mixed", n, 0, [[0, n], _three(n)], oracle)
        _matrix(path, "mixed", n, 0, [None], oracle, many=True)  # > 1023 dict blobs
    else:
        _matrix(path, "mixed", n, GRID, [None, _three(n)] if n >= 3 else [None], oracle)
        if n > 4096:  # the grid kernels without the flag
            _matrix(path, "mixed", n, 0, [None, _three(n)], oracle)


WHOLE = [(p, k, n) for k in ("hot", "distinct", "all_dict") for n in dc.WHOLE_N
         for p in ("lds", "small", "grid")]


@pytest.mark.parametrize("path,kind,n", WHOLE, ids=[f"{p}-{k}-{n}" for p, k, n in WHOLE])
def test_whole_layer_cases(path, kind, n, oracle):
    """One slot every lane races on (hot), no two chunks equal and a layer
    total of exactly 2^32 at n = 256 (distinct), no NEW chunk at all, so
    own_blob_index = 0xFFFFFFFF (all_dict)."""
    if path == "lds":
        _matrix("lds256" if n <= 256 else "lds1024", kind, n, 0, [None], oracle)
    elif path == "small":
        _matrix(path, kind, n, 0, [[0, n], _three(n)], oracle)
    else:
        _matrix(path, kind, n, GRID, [None, _three(n)], oracle)

