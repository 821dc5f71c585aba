"""Dict fold (ngpu_dict_fold / ngpu_dict_extend_device, csrc/dict.hip +
csrc/dict_fold.hip) on the GPU.

The expectation everywhere is what the header defines: the base's rows followed by
one row per NEW chunk of the call's result table, built on the host by a numpy
model (_model) from the same tables.  Every case is compared three ways, byte for
byte through ngpu_dict_export: fold(base), base.extend(model rows), and the model
rows appended to base.export().

  1  sizes at which a wave, a keep word, a workgroup or a scan tile ends, for every
     NEW pattern; the first fold forks, a second one appends in place
  2  layers: counts, empty layers, layers without a NEW chunk, cuts on and inside
     a keep word, blob counts and blob-table rows
  3  share / fork, older handles blind to in-place folds, retire before and after
  4  placements and their refusals
  5  device-side refusals (kinds, lengths, layer cuts) leave the base as it was
  6  extend_device
  7  real digests end to end, one layer and 40 layers
  8  in-place folds while dedup kernels probe the base on another stream
"""
import threading

import numpy as np
import pytest

import dedup_cases as dc
import nydus_gpu
from nydus_gpu import rafs

pytestmark = pytest.mark.gpu

CS = 0x10000
NEW, INTRA, DICT, DIGESTED, UNHASHED = 0, 1, 2, 3, 4
GRID = nydus_gpu.FLAG_GRID_STAGES
T = 256 * 64  # one scan tile: kRetireScanTile keep words of 64 chunks
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def _fork_caps(m, k):
    """dict_grow_plan's fork: record and table capacity for m + k entries."""
    n = m + k
    want = n + max(k, n // 2)
    return want, _pow2(2 * want + 16)


def _same_rows(got, exp, tag):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for f in exp.dtype.names if len(exp) else ():
        bad = np.flatnonzero((got[f] != exp[f]).reshape(len(exp), -1).any(axis=1))
        assert not len(bad), f"{tag}: {f} differs in {len(bad)} rows, first {bad[0]}: " \
                             f"got {got[f][bad[0]]}, expected {exp[f][bad[0]]}"
    assert got.tobytes() == exp.tobytes(), tag


def _tables(rng, n, new, cs=CS):
    """A result table and descriptors as a dedup call leaves them, written from
    numpy: `new` marks the NEW chunks, the others are INTRA or DICT; every field a
    fold must not read is noise, index is arbitrary and offsets go past 2^32."""
    res = np.zeros(n, nydus_gpu.RESULT_DTYPE)
    res["digest"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    res["kind"] = np.where(new, NEW, rng.integers(1, 3, n))
    res["index"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    res["ref"] = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    res["blob_index"] = rng.integers(0, 1 << 20, n)
    res["dict_blob"] = rng.integers(0, 1 << 20, n)
    res["uncompressed_offset"] = rng.integers(0, 1 << 44, n, dtype=np.uint64)
    ch = np.zeros(n, nydus_gpu.CHUNK_DTYPE)
    ch["offset"] = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    ch["length"] = rng.integers(1, cs + 1, n)
    ch["file_index"] = rng.integers(0, 1 << 20, n)
    ch["file_offset"] = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    if n:
        ch["length"][rng.integers(0, n)] = cs  # the largest length a record carries
    return res, ch


def _model(res, ch, first=None, placements=None):
    """The host rows the header defines -> (80-B rows, b).  A chunk's layer is the
    last one that starts at or before it; a layer's blob is its rank among the
    layers that hold a NEW chunk."""
    n = len(res)
    new = res["kind"] == NEW
    cuts = np.asarray([0, n] if first is None else first, np.int64)
    L = len(cuts) - 1
    layer = np.searchsorted(cuts[1:], np.arange(n), side="right")
    has = np.bincount(layer[new], minlength=L)[:L] > 0
    rank = np.cumsum(has) - has
    rows = np.zeros(int(new.sum()), rafs.CHUNK_INFO_DTYPE)
    rows["block_id"] = res["digest"][new]
    rows["uncompressed_size"] = ch["length"][new]
    rows["blob_index"] = rank[layer[new]]
    rows["index"] = res["index"][new]
    rows["uncompressed_offset"] = res["uncompressed_offset"][new]
    if placements is None:
        rows["compressed_size"] = rows["uncompressed_size"]
    else:
        for f in ("compressed_offset", "compressed_size", "flags"):
            rows[f] = placements[f]
    return rows, int(has.sum())


def _places(rng, k):
    p = np.zeros(k, nydus_gpu.DICT_PLACE_DTYPE)
    p["compressed_offset"] = rng.integers(0, 1 << 44, k, dtype=np.uint64)
    p["compressed_size"] = rng.integers(1, 1 << 16, k)
    p["flags"] = rng.integers(0, 2, k)
    return p


def _appended(base_rows, base_blobs, rows):
    r = rows.copy()
    r["blob_index"] += base_blobs
    return np.concatenate([base_rows, r])


def _base_arrays(rng, m, nb=1):
    """m random rows as create_device's arrays -> (device tensors, the 80-B rows)."""
    rows = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
    rows["block_id"] = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    rows["uncompressed_size"] = rng.integers(1, CS + 1, m)
    rows["blob_index"] = rng.integers(0, nb, m)
    rows["index"] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    rows["uncompressed_offset"] = rng.integers(0, 1 << 44, m, dtype=np.uint64)
    rows["compressed_size"] = rows["uncompressed_size"]  # what a dict without placements exports
    return _arrays(rows), rows


def _arrays(rows):
    return [_dev(np.ascontiguousarray(rows[f])) for f in
            ("block_id", "uncompressed_size", "blob_index", "index", "uncompressed_offset")]


def _create_device(eng, arrs, m, nb):
    import torch
    torch.cuda.synchronize()
    dg, us, bl, ix, uo = arrs
    return eng.dict_create_device(dg.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), m, nb,
                                  d_uoff=uo.data_ptr())


def _fold(d, res, ch, first=None, placements=None, blobs=None):
    """Upload the tables (and cuts) and fold them; -> the new handle."""
    import torch
    d_res, d_ch = _dev(res), _dev(ch)
    d_first = None if first is None else _dev(np.asarray(first, np.uint64))
    torch.cuda.synchronize()
    return d.fold(d_res.data_ptr(), d_ch.data_ptr(), len(res),
                  d_layer_first=0 if d_first is None else d_first.data_ptr(),
                  n_layers=1 if first is None else len(first) - 1, placements=placements, blobs=blobs)


def _patterns(n, rng):
    idx = np.arange(n)
    yield "all", np.ones(n, bool)
    yield "none", np.zeros(n, bool)
    yield "every other", idx % 2 == 0
    yield "runs of 64", (idx // 64) % 2 == 0
    yield "first", idx == 0
    yield "last", idx == n - 1
    yield "random 30%", rng.random(n) < 0.3


def _probe(d, d_q, nq):
    import torch
    hits = torch.zeros(max(nq, 1) * 24, dtype=torch.uint8, device="cuda")
    d.probe_device(d_q.data_ptr(), 32, nq, hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(nydus_gpu.HIT_DTYPE)[:nq]


def _dedup(eng, d, digests, lengths, stream=0):
    """One dedup call against d over caller-supplied digests -> (device result
    table, device descriptors, host copy, stats)."""
    import torch
    n = len(lengths)
    ch = np.zeros(n, nydus_gpu.CHUNK_DTYPE)
    ch["length"] = lengths
    ch["file_index"] = np.arange(n)
    rec0 = np.zeros(n, nydus_gpu.RESULT_DTYPE)
    rec0["digest"] = digests
    rec0["kind"] = DIGESTED
    d_ch, out = _dev(ch), _dev(rec0)
    torch.cuda.synchronize()
    eng.set_dict(d)
    st = eng.dedup_device(d_ch.data_ptr(), n, out.data_ptr(), want_stats=True)
    torch.cuda.synchronize()
    return out, d_ch, out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE), st


# ---- 1: sizes and NEW patterns ----------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_fold_sizes_and_patterns_three_ways(n):
    """A create_device base of 100 rows; the first fold forks (capacities as
    dict_grow_plan says), a second fold of the same table appends in place."""
    rng = np.random.default_rng(7000 + n)
    m0 = 100
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        arrs, rows0 = _base_arrays(rng, m0)
        base = _create_device(eng, arrs, m0, 1)
        for name, new in _patterns(n, rng):
            res, ch = _tables(rng, n, new)
            rows, b = _model(res, ch)
            k = len(rows)
            assert k == int(new.sum()) and b == (1 if k else 0)
            f1 = _fold(base, res, ch)
            f2 = _fold(f1, res, ch)
            x1 = base.extend(rows)
            x2 = x1.extend(rows)
            exp1 = _appended(rows0, 1, rows)
            exp2 = _appended(exp1, 1 + b, rows)
            for tag, f, x, exp, nb in (("fork", f1, x1, exp1, 1 + b), ("share", f2, x2, exp2, 1 + 2 * b)):
                got, gtbl = f.export()
                via, _ = x.export()
                _same_rows(got, exp, f"n={n} {name} {tag} fold vs model")
                _same_rows(via, exp, f"n={n} {name} {tag} extend vs model")
                assert gtbl is None
                fi, xi = f.info(), x.info()
                assert fi == xi, (name, tag, fi, xi)
                assert (fi["entries"], fi["blobs"]) == (m0 + len(exp) - m0, nb), (name, tag, fi)
            i1, i2 = f1.info(), f2.info()
            if k:
                assert (i1["record_capacity"], i1["table_capacity"]) == _fork_caps(m0, k), (name, i1)
                assert not i1["shares_base_storage"] and i2["shares_base_storage"], name
                assert (i2["record_capacity"], i2["table_capacity"]) == (i1["record_capacity"], i1["table_capacity"])
            else:  # k == 0: a handle equal to base
                assert i1["entries"] == m0 and i1["record_capacity"] == m0
            back, _ = base.export()  # the base is as it was
            _same_rows(back, rows0, f"n={n} {name} base")
            for h in (f1, f2, x1, x2):
                h.release()
        base.release()
        eng.device_status()


# ---- 2: layers --------------------------------------------------------------------------
def _cuts(rng, n, L):
    """L + 1 layer cuts of n chunks: empty layers at the front, in the middle and at
    the end, one cut exactly on a keep word and one inside it."""
    inner = np.sort(rng.integers(0, n + 1, max(L - 1, 0)))
    first = np.concatenate([[0], inner, [n]]).astype(np.int64)
    if L >= 3:
        first[1] = 0            # an empty first layer
        first[L - 1] = n        # an empty last layer
    if L >= 64:
        first[L // 2] = first[L // 2 + 1]  # an empty layer in the middle
        first[2], first[3] = 64, 64 + 37   # on a keep word, inside one
    first = np.maximum.accumulate(first)
    first[-1] = n
    return np.minimum(first, n)


@pytest.mark.parametrize("L", [1, 2, 3, 64, 257, 1025])
def test_fold_layers_blob_ranks_and_tables(L):
    """Layers without a NEW chunk stand on both sides of layers with one (where
    blob ranks must skip); the base has a blob table and placements, so the call
    brings b table rows and k placement rows, and the export carries both."""
    rng = np.random.default_rng(8000 + L)
    n = T + 1000  # more than one scan tile
    first = _cuts(rng, n, L)
    layer = np.searchsorted(first[1:], np.arange(n), side="right")
    # every third layer has no NEW chunk
    barren = np.arange(L) % 3 == 2
    new = (rng.random(n) < 0.4) & ~barren[layer]
    res, ch = _tables(rng, n, new)
    m0 = 50
    base_rows = np.zeros(m0, rafs.CHUNK_INFO_DTYPE)
    base_rows["block_id"] = rng.integers(0, 256, (m0, 32), dtype=np.uint8)
    base_rows["uncompressed_size"] = CS
    base_rows["blob_index"] = rng.integers(0, 2, m0)
    base_rows["compressed_size"] = 999
    tbl0 = rafs.make_blob_table([f"{i:064x}" for i in range(2)], CS)
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        base = eng.dict_create(base_rows, tbl0)
        k = int(new.sum())
        pl = _places(rng, k)
        rows, b = _model(res, ch, first, pl)
        if L >= 3:
            assert 0 < b < L and len(set(rows["blob_index"])) == b == int(rows["blob_index"].max()) + 1
        tbl = rafs.make_blob_table([f"{0xAB00 + i:064x}" for i in range(b)], CS)
        f = _fold(base, res, ch, first if L > 1 else None, pl, tbl)
        x = base.extend(rows, tbl)
        exp = _appended(base_rows, 2, rows)
        got, gtbl = f.export()
        via, vtbl = x.export()
        _same_rows(got, exp, f"L={L} fold vs model")
        _same_rows(via, exp, f"L={L} extend vs model")
        want_tbl = np.ascontiguousarray(tbl0).tobytes() + np.ascontiguousarray(tbl).tobytes()
        assert gtbl == vtbl == want_tbl
        assert f.info() == x.info() and f.info()["blobs"] == 2 + b
        # a table of the wrong row count is refused: n_blobs == b
        for wrong in (b - 1, b + 1):
            if wrong > 0:
                with pytest.raises(nydus_gpu.NgpuError) as ei:
                    _fold(base, res, ch, first if L > 1 else None, pl,
                          rafs.make_blob_table([f"{i:064x}" for i in range(wrong)], CS))
                assert ei.value.code == nydus_gpu.EINVAL
        # given cuts with n_layers == 1 are one layer
        if L == 1:
            g = _fold(base, res, ch, [0, n], pl, tbl)
            assert g.export()[0].tobytes() == got.tobytes()
            g.release()
        for h in (f, x, base):
            h.release()
        eng.device_status()


# ---- 3: share, fork, older handles, retire ----------------------------------------------
def test_share_fork_older_handles_and_retire():
    rng = np.random.default_rng(31)
    m0, n = 1000, 900
    R1 = np.zeros(m0, rafs.CHUNK_INFO_DTYPE)
    R1["block_id"] = rng.integers(0, 256, (m0, 32), dtype=np.uint8)
    R1["uncompressed_size"] = CS
    R1["compressed_size"] = rng.integers(1, 1 << 16, m0)
    R1["compressed_offset"] = rng.integers(0, 1 << 40, m0)
    # two layers' worth of digests: half of each are rows of R1 (DICT), the rest new
    digs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(3)]
    for i, d in enumerate(digs):
        d[::2] = R1["block_id"][i * 250:i * 250 + n // 2]
    lens = rng.integers(1, CS + 1, n)
    lens[::2] = CS  # a dict row answers for its own size only
    nC = 400
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        d = eng.dict_create(R1)
        info = d.info()
        assert (info["record_capacity"], info["table_capacity"], info["shares_base_storage"]) == (m0, 2048, False)
        # layer A through a real dedup against d, folded from its device tables
        outA, chA, hostA, stA = _dedup(eng, d, digs[0], lens)
        assert stA["dict_chunks"] == n // 2 and stA["new_chunks"] == n // 2
        chA_h = chA.cpu().numpy().view(nydus_gpu.CHUNK_DTYPE)
        kA = stA["new_chunks"]
        plA = _places(rng, kA)
        f1 = d.fold(outA.data_ptr(), chA.data_ptr(), n, placements=plA)
        rowsA, bA = _model(hostA, chA_h, None, plA)
        assert bA == 1 and len(rowsA) == kA
        i1 = f1.info()
        assert (i1["record_capacity"], i1["table_capacity"]) == _fork_caps(m0, kA) and not i1["shares_base_storage"]
        exp1 = _appended(R1, 1, rowsA)
        _same_rows(f1.export()[0], exp1, "first fold forks")
        # what f1 answers before anything is appended behind it
        q = np.concatenate([digs[1], digs[0][:50], R1["block_id"][:50]])
        d_q = _dev(q)
        hits_before = _probe(f1, d_q, len(q)).tobytes()
        outB, chB, hostB, stB = _dedup(eng, f1, digs[1], lens)
        assert stB["new_chunks"] == n // 2
        # layer B's NEW chunks are the very digests f1 misses: folded in place
        plB = _places(rng, stB["new_chunks"])
        f2 = f1.fold(outB.data_ptr(), chB.data_ptr(), n, placements=plB)
        i2 = f2.info()
        assert i2["shares_base_storage"]
        assert (i2["record_capacity"], i2["table_capacity"]) == (i1["record_capacity"], i1["table_capacity"])
        rowsB, _ = _model(hostB, chB.cpu().numpy().view(nydus_gpu.CHUNK_DTYPE), None, plB)
        exp2 = _appended(exp1, 2, rowsB)
        _same_rows(f2.export()[0], exp2, "second fold appends in place")
        # the older handle is blind to the append: probes and a dedup answer as before
        assert _probe(f1, d_q, len(q)).tobytes() == hits_before
        miss = _probe(f1, d_q, len(q))["entry"][1:n:2]
        assert (miss == nydus_gpu.MISS).all() and (_probe(f2, d_q, len(q))["entry"][:n] != nydus_gpu.MISS).all()
        _, _, againB, stB2 = _dedup(eng, f1, digs[1], lens)
        assert againB.tobytes() == hostB.tobytes() and stB2 == stB
        _, _, viaF2, st2 = _dedup(eng, f2, digs[1], lens)
        assert st2["new_chunks"] == 0 and st2["dict_chunks"] == n
        eng.set_dict(None)
        # a fold after a retire appends in place (a retire leaves s / 2 slots of room)
        r = f2.retire([0])
        s = r.entries
        assert s == len(rowsA) + len(rowsB) and r.info()["blobs"] == 2
        outC, chC, hostC, stC = _dedup(eng, r, digs[2][:nC], lens[:nC])
        eng.set_dict(None)
        assert 0 < stC["new_chunks"] <= s // 2
        plC = _places(rng, stC["new_chunks"])
        g = r.fold(outC.data_ptr(), chC.data_ptr(), nC, placements=plC)
        assert g.info()["shares_base_storage"] and g.info()["record_capacity"] == r.info()["record_capacity"]
        rowsC, _ = _model(hostC, chC.cpu().numpy().view(nydus_gpu.CHUNK_DTYPE), None, plC)
        _same_rows(g.export()[0], _appended(r.export()[0], 2, rowsC), "fold after retire")
        # a retire after a fold drops the folded blob: back to the base's rows
        h = f1.retire([1])
        _same_rows(h.export()[0], R1, "retire of the folded blob")
        assert h.info()["blobs"] == 1
        for x in (h, g, r, f2, f1, d):
            x.release()
        eng.device_status()


# ---- 4: placements ----------------------------------------------------------------------
def test_placements_kept_defaulted_and_refused():
    rng = np.random.default_rng(41)
    n = 300
    res, ch = _tables(rng, n, rng.random(n) < 0.5)
    k = int((res["kind"] == NEW).sum())
    pl = _places(rng, k)
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        recs = np.zeros(40, rafs.CHUNK_INFO_DTYPE)
        recs["block_id"] = rng.integers(0, 256, (40, 32), dtype=np.uint8)
        recs["uncompressed_size"] = 4096
        recs["compressed_size"] = 123
        recs["compressed_offset"] = np.arange(40) * 4096
        recs["flags"] = 1
        with_pl = eng.dict_create(recs)                 # keeps placements
        arrs, rows0 = _base_arrays(rng, 40)
        without = _create_device(eng, arrs, 40, 1)      # keeps none
        empty = eng.dict_create(np.zeros(0, rafs.CHUNK_INFO_DTYPE))
        # base from 80-B records + placements: the export carries them
        f = _fold(with_pl, res, ch, placements=pl)
        rows, _ = _model(res, ch, None, pl)
        _same_rows(f.export()[0], _appended(recs, 1, rows), "placements kept")
        x = with_pl.extend(rows)
        assert x.export()[0].tobytes() == f.export()[0].tobytes()
        # base from create_device, none given: csize = usize, offset 0, flags 0
        g = _fold(without, res, ch)
        rows_np, _ = _model(res, ch)
        got = g.export()[0]
        _same_rows(got, _appended(rows0, 1, rows_np), "no placements")
        assert (got["compressed_size"] == got["uncompressed_size"]).all()
        assert not got["compressed_offset"].any() and not got["flags"].any()
        # an empty base goes with either
        e1, e2 = _fold(empty, res, ch, placements=pl), _fold(empty, res, ch)
        _same_rows(e1.export()[0], rows, "empty base, placements")
        _same_rows(e2.export()[0], rows_np, "empty base, none")
        # the refusals; nothing is dropped silently
        for base, kw, what in ((with_pl, {}, "base keeps placements, none given"),
                               (without, {"placements": pl}, "base keeps none, some given"),
                               (with_pl, {"placements": pl[:-1]}, "n_placements == k - 1"),
                               (with_pl, {"placements": np.concatenate([pl, pl[:1]])}, "n_placements == k + 1"),
                               (empty, {"placements": pl[:1]}, "n_placements != k on an empty base")):
            before = base.export()[0].tobytes()
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                _fold(base, res, ch, **kw)
            assert ei.value.code == nydus_gpu.EINVAL, what
            assert base.export()[0].tobytes() == before and not base.info()["shares_base_storage"]
        # k == 0: a handle equal to base, whatever it keeps; an empty list is fine
        none_new, ch0 = _tables(rng, 64, np.zeros(64, bool))
        for base in (with_pl, without):
            z = _fold(base, none_new, ch0)
            z2 = _fold(base, none_new, ch0, placements=np.zeros(0, nydus_gpu.DICT_PLACE_DTYPE))
            assert z.export()[0].tobytes() == z2.export()[0].tobytes() == base.export()[0].tobytes()
            assert z.info()["entries"] == base.info()["entries"] and z.info()["blobs"] == base.info()["blobs"]
            z.release()
            z2.release()
        for h in (f, x, g, e1, e2, with_pl, without, empty):
            h.release()
        eng.device_status()


# ---- 5: device-side refusals ------------------------------------------------------------
def test_device_side_refusals_leave_the_base_untouched():
    """Every refused table is one the kernels reject by their kind and bounds checks
    before any dependent access.  After each refusal the tip still answers as
    before, and a following valid fold appends in place: no record slot was
    reserved by the refused call."""
    rng = np.random.default_rng(51)
    n = T + 300
    res, ch = _tables(rng, n, rng.random(n) < 0.3)
    first = [0, 1000, 1000, T, n]
    q = np.concatenate([res["digest"][:200], rng.integers(0, 256, (50, 32), dtype=np.uint8)])
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        arrs, rows0 = _base_arrays(rng, 2000)
        base = _create_device(eng, arrs, 2000, 1)
        seedr, seedc = _tables(rng, 500, np.ones(500, bool))
        tip = _fold(base, seedr, seedc)  # a tip with room: 1250 free slots at least
        assert tip.info()["record_capacity"] - tip.entries >= 1250
        d_q = _dev(q)
        answers = _probe(tip, d_q, len(q)).tobytes()
        rows_tip = tip.export()[0].tobytes()

        def refused(r, c, cuts, needle):
            nonlocal tip
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                _fold(tip, r, c, cuts)
            assert ei.value.code == nydus_gpu.EINVAL and needle in str(ei.value), (needle, str(ei.value))
            assert _probe(tip, d_q, len(q)).tobytes() == answers
            assert tip.export()[0].tobytes() == rows_tip
            ok_r, ok_c = _tables(rng, 30, np.ones(30, bool))
            nxt = _fold(tip, ok_r, ok_c)  # a valid fold right after: in place
            assert nxt.info()["shares_base_storage"] and nxt.entries == tip.entries + 30
            _same_rows(nxt.export()[0][-30:], _appended(rows0[:0], tip.info()["blobs"], _model(ok_r, ok_c)[0]),
                       "fold after a refusal")
            nxt.release()
            # (the 30 slots stay dead on the storage; the next valid fold forks or fits)
            fresh = _fold(base, seedr, seedc)
            tip.release()
            tip = fresh

        for kind in (DIGESTED, UNHASHED, 7):
            for at in (0, n // 2, n - 1):
                bad = res.copy()
                bad["kind"][at] = kind
                if at != n - 1:
                    bad["kind"][n - 1] = 9  # a later one too: the first is named
                refused(bad, ch, first, f"chunk {at} ")
        new_at = int(np.flatnonzero(res["kind"] == NEW)[len(res) // 8])
        for length in (0, CS + 1):
            bad = ch.copy()
            bad["length"][new_at] = length
            refused(res, bad, first, f"NEW chunk {new_at} ")
        # a wrong length on a chunk that is not NEW is not read
        other_at = int(np.flatnonzero(res["kind"] != NEW)[3])
        okc = ch.copy()
        okc["length"][other_at] = 0
        f = _fold(tip, res, okc, first)
        assert f.entries == tip.entries + int((res["kind"] == NEW).sum())
        f.release()
        for cuts in ([0, 1000, 999, T, n], [0, 1000, 1000, T, n - 1], [0, 1000, 1000, T, n + 1],
                     [1, 1000, 1000, T, n], [0, n + 5, n + 5, n + 5, n]):
            refused(res, ch, cuts, "layer_first")
        tip.release()
        base.release()
        eng.device_status()


# ---- 6: extend_device -------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_extend_device_equals_extend_of_the_same_rows(n):
    """A create_device dict extended twice from device arrays, forking and then in
    place, against extend() of the same rows as 80-B records."""
    import torch
    rng = np.random.default_rng(9000 + n)
    m0, nb_new = 100, 3
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        arrs, rows0 = _base_arrays(rng, m0, 2)
        base = _create_device(eng, arrs, m0, 2)
        _, rows = _base_arrays(rng, n, nb_new)
        if n:
            rows["blob_index"][rng.integers(0, n)] = nb_new - 1  # so that extend() counts nb_new blobs too
        dg, us, bl, ix, uo = _arrays(rows)
        torch.cuda.synchronize()
        nb = nb_new if n else 0
        f1 = base.extend_device(dg.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), n, nb, d_uoff=uo.data_ptr())
        f2 = f1.extend_device(dg.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr(), n, nb, d_uoff=uo.data_ptr())
        x1 = base.extend(rows)
        x2 = x1.extend(rows)
        exp1 = _appended(rows0, 2, rows)
        exp2 = _appended(exp1, 2 + nb, rows)
        for tag, f, x, exp in (("fork", f1, x1, exp1), ("share", f2, x2, exp2)):
            _same_rows(f.export()[0], exp, f"n={n} {tag} extend_device vs model")
            _same_rows(x.export()[0], exp, f"n={n} {tag} extend vs model")
            assert f.info() == x.info(), (tag, f.info(), x.info())
        if n:
            i1, i2 = f1.info(), f2.info()
            assert (i1["record_capacity"], i1["table_capacity"]) == _fork_caps(m0, n)
            assert not i1["shares_base_storage"] and i2["shares_base_storage"]
            # probes: ids m + position, first entry wins
            q = np.concatenate([rows["block_id"][:64], rows0["block_id"][:8]])
            hits = _probe(f2, _dev(q), len(q))
            assert (hits["entry"][:min(n, 64)] == m0 + np.arange(min(n, 64))).all()
            assert (hits["blob"][:min(n, 64)] == rows["blob_index"][:64] + 2).all()
            # without offsets and indices: zeros
            f3 = base.extend_device(dg.data_ptr(), us.data_ptr(), bl.data_ptr(), 0, n, nb)
            bare = rows.copy()
            bare["index"] = 0
            bare["uncompressed_offset"] = 0
            _same_rows(f3.export()[0], _appended(rows0, 2, bare), "no index / uoff arrays")
            f3.release()
        else:
            assert f1.info()["entries"] == m0 and f1.info()["blobs"] == 2
        for h in (f1, f2, x1, x2, base):
            h.release()
        eng.device_status()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_create_device_with_global_ids_equals_create_of_the_same_rows(n):
    """create_device with a global id array (the SoA pack kernel's other gid source),
    with and without the index / offset arrays, against create() of the same rows as
    80-B records: the same exported rows, and every probe hit the host-path dict's
    with its entry (a position there) looked up in the id array."""
    import torch
    rng = np.random.default_rng(9500 + n)
    nb = 3
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        (dg, us, bl, ix, uo), rows = _base_arrays(rng, n, nb)
        gid = rng.permutation(n).astype(np.uint32) + 1000
        d_gid = _dev(gid)
        q = _dev(np.concatenate([rows["block_id"], rng.integers(0, 256, (5, 32), dtype=np.uint8)]))
        torch.cuda.synchronize()
        bare = rows.copy()
        bare["index"] = 0
        bare["uncompressed_offset"] = 0
        for tag, exp, p_ix, p_uo in (("all arrays", rows, ix.data_ptr(), uo.data_ptr()),
                                     ("no index / uoff arrays", bare, 0, 0)):
            d = eng.dict_create_device(dg.data_ptr(), us.data_ptr(), bl.data_ptr(), p_ix, n, nb,
                                       d_uoff=p_uo, d_gid=d_gid.data_ptr())
            host = eng.dict_create(exp)
            _same_rows(d.export()[0], exp, f"n={n} {tag}: export vs the rows")
            _same_rows(d.export()[0], host.export()[0], f"n={n} {tag}: export vs the host path")
            got, ref = _probe(d, q, n + 5), _probe(host, q, n + 5)
            hit = ref["entry"] != 0xFFFFFFFF
            assert hit[:n].all() and not hit[n:].any()
            want = ref.copy()
            want["entry"][hit] = gid[ref["entry"][hit]]
            assert got.tobytes() == want.tobytes(), f"n={n} {tag}: probe hits"
            d.release()
            host.release()
        eng.device_status()


def test_extend_device_refusals():
    import torch
    rng = np.random.default_rng(61)
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        _, rows = _base_arrays(rng, 20)
        dg, us, bl, ix, uo = _arrays(rows)
        torch.cuda.synchronize()
        args = (dg.data_ptr(), us.data_ptr(), bl.data_ptr(), ix.data_ptr())
        with_table = eng.dict_create(rows, rafs.make_blob_table(["ab" * 32], CS))
        with_place = eng.dict_create(rows)
        arrs, _ = _base_arrays(rng, 20)
        plain = _create_device(eng, arrs, 20, 1)
        for base, what in ((with_table, "a base with a blob table"), (with_place, "a base with placements")):
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                base.extend_device(*args, 20, 1)
            assert ei.value.code == nydus_gpu.EINVAL, what
            same = base.extend_device(*args, 0, 0)  # n == 0: a handle equal to base
            assert same.export()[0].tobytes() == base.export()[0].tobytes()
            assert same.export()[1] == base.export()[1]
            same.release()
        with pytest.raises(nydus_gpu.NgpuError) as ei:  # 2^20 blobs in all, not one more
            plain.extend_device(*args, 20, 1 << 20)
        assert ei.value.code == nydus_gpu.EINVAL
        top = plain.extend_device(*args, 20, (1 << 20) - 1)
        assert top.info()["blobs"] == 1 << 20
        with pytest.raises(nydus_gpu.NgpuError):
            top.extend_device(*args, 20, 1)
        for h in (top, plain, with_place, with_table):
            h.release()
        eng.device_status()


# ---- 7: real digests, end to end --------------------------------------------------------
def _layer(rng, n, max_len, reuse=None, share=0.0):
    """A layer of n chunks of random bytes -> (data, CHUNK_DTYPE); a `share` of its
    chunks repeat chunks of `reuse` = (data, chunks), and a few repeat its own."""
    parts, lens = [], []
    for i in range(n):
        if reuse is not None and rng.random() < share:
            rd, rc = reuse
            j = int(rng.integers(0, len(rc)))
            b = rd[int(rc["offset"][j]):int(rc["offset"][j]) + int(rc["length"][j])]
        elif i > 4 and rng.random() < 0.1:
            b = parts[int(rng.integers(0, i))]
        else:
            b = rng.integers(0, 256, int(rng.integers(1, max_len + 1)), dtype=np.uint8)
        parts.append(b)
        lens.append(len(b))
    ch = np.zeros(n, nydus_gpu.CHUNK_DTYPE)
    ch["length"] = lens
    ch["offset"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    ch["file_index"] = np.arange(n)
    return np.concatenate(parts), ch


@pytest.mark.parametrize("flags", [GRID, 0], ids=["grid", "fused"])
def test_fold_a_processed_layer_then_dedup_the_next(oracle, flags):
    import torch
    rng = np.random.default_rng(71 + flags)
    nA, nB = 600, 500
    dataA, chA = _layer(rng, nA, 3000)
    dataB, chB = _layer(rng, nB, 3000, (dataA, chA), 0.3)
    with nydus_gpu.Engine(chunk_size=CS, flags=flags) as eng:
        arrs, rows0 = _base_arrays(rng, 64)
        base = _create_device(eng, arrs, 64, 1)
        eng.set_dict(base)
        d_data, d_ch = _dev(dataA), _dev(chA)
        out = torch.zeros(nA * 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stA = eng.process_device(d_data.data_ptr(), len(dataA), d_ch.data_ptr(), nA, out.data_ptr(), want_stats=True)
        torch.cuda.synchronize()
        hostA = out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
        assert np.array_equal(hostA["digest"], oracle.digest_chunks(dataA, chA, "blake3"))
        assert stA["new_chunks"] > 0 and stA["intra_chunks"] > 0
        f = base.fold(out.data_ptr(), d_ch.data_ptr(), nA)
        rows, b = _model(hostA, chA)
        assert b == 1 and len(rows) == stA["new_chunks"] == f.entries - 64
        all_rows = _appended(rows0, 1, rows)
        _same_rows(f.export()[0], all_rows, "folded layer")
        # the next layer against the folded dict == the oracle over base rows ++ folded rows
        eng.set_dict(f)
        d_dataB, d_chB = _dev(dataB), _dev(chB)
        outB = torch.zeros(nB * 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stB = eng.process_device(d_dataB.data_ptr(), len(dataB), d_chB.data_ptr(), nB, outB.data_ptr(), want_stats=True)
        torch.cuda.synchronize()
        got = outB.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
        dig = oracle.digest_chunks(dataB, chB, "blake3")
        dec, _ = oracle.dedup(dig, chB["length"], all_rows["block_id"], all_rows["uncompressed_size"],
                              all_rows["blob_index"], all_rows["index"], dict_uoff=all_rows["uncompressed_offset"])
        assert np.array_equal(got["digest"], dig)
        for fld in ("kind", "index", "ref", "blob_index", "uncompressed_offset"):
            assert np.array_equal(got[fld], dec[fld]), fld
        hit = got["kind"] == DICT
        assert 100 < hit.sum() == stB["dict_chunks"] < nB
        assert (got["dict_blob"][hit] == 1).all() and (got["ref"][hit] >= 64).all()
        eng.set_dict(None)
        f.release()
        base.release()
        eng.device_status()


def test_fold_forty_layers_of_one_call():
    """40 small layers through one process_layers_device call, folded in one call;
    the same 40 layers again come back all DICT, dict_blob naming each layer's
    blob rank."""
    import torch
    rng = np.random.default_rng(81)
    L = 40
    layers = [_layer(rng, int(rng.integers(5, 40)), 2000) for _ in range(L)]
    data = np.concatenate([d for d, _ in layers])
    chs, first, off = [], [0], 0
    for d, c in layers:
        c = c.copy()
        c["offset"] += off
        off += len(d)
        chs.append(c)
        first.append(first[-1] + len(c))
    ch = np.concatenate(chs)
    n = len(ch)
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        arrs, rows0 = _base_arrays(rng, 64, 2)
        base = _create_device(eng, arrs, 64, 2)
        d_data, d_ch, d_first = _dev(data), _dev(ch), _dev(np.asarray(first, np.uint64))

        def run(d):
            eng.set_dict(d)
            out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            eng.process_layers_device(d_data.data_ptr(), len(data), d_ch.data_ptr(), n, out.data_ptr(),
                                      d_first.data_ptr(), L)
            torch.cuda.synchronize()
            eng.device_status()
            return out, out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)

        out, host = run(base)
        assert set(np.unique(host["kind"])) <= {NEW, INTRA}
        f = base.fold(out.data_ptr(), d_ch.data_ptr(), n, d_layer_first=d_first.data_ptr(), n_layers=L)
        rows, b = _model(host, ch, first)
        assert b == L and f.info()["blobs"] == 2 + L
        all_rows = _appended(rows0, 2, rows)
        _same_rows(f.export()[0], all_rows, "40 layers")
        _, again = run(f)
        assert (again["kind"] == DICT).all()
        layer = np.searchsorted(np.asarray(first[1:]), np.arange(n), side="right")
        assert np.array_equal(again["dict_blob"], 2 + layer)
        # each hit names the first record with its digest
        firsts = {}
        for j, dgst in enumerate(all_rows["block_id"]):
            firsts.setdefault(bytes(dgst), j)
        assert np.array_equal(again["ref"], [firsts[bytes(x)] for x in host["digest"]])
        eng.set_dict(None)
        f.release()
        base.release()


# ---- 8: folds under load ----------------------------------------------------------------
def test_in_place_folds_while_dedup_probes_the_base():
    """One thread runs 40 dedup calls against x1 on a side stream while another
    chains 16 in-place folds on top of x1 whose NEW chunks are the very digests x1
    misses: every dedup equals x1's answer, the final handle equals its model."""
    import torch
    case = dc.get("mixed", 4097, 4096, True)
    rng = np.random.default_rng(91)
    eng = nydus_gpu.Engine(chunk_size=dc.CHUNK_SIZE)
    try:
        dd, ds, db, di, duoff, nb = case.dict
        R1 = np.zeros(len(ds), rafs.CHUNK_INFO_DTYPE)
        R1["block_id"], R1["uncompressed_size"], R1["blob_index"] = dd, ds, db
        R1["index"], R1["uncompressed_offset"] = di, duoff
        R1["compressed_size"] = R1["uncompressed_size"]
        b = _create_device(eng, _arrays(R1), len(R1), nb)
        seedr, seedc = _tables(rng, 2000, np.ones(2000, bool), dc.CHUNK_SIZE)
        x1 = _fold(b, seedr, seedc)
        m1 = len(R1) + 2000
        have = {bytes(x) for x in R1["block_id"]}
        pool = np.concatenate([case.digests, dc.get("mixed", 1025, 4096, True).digests])
        fresh = np.stack(list({bytes(x): x for x in pool if bytes(x) not in have}.values()))[:400]
        assert len(fresh) == 400 and x1.info()["record_capacity"] >= m1 + 800
        # 16 tables of 50 chunks: every other one NEW, half of those x1's misses
        tabs = []
        for i in range(16):
            r, c = _tables(rng, 50, np.arange(50) % 2 == 0, dc.CHUNK_SIZE)
            r["digest"][0::2] = fresh[25 * i:25 * i + 25]
            tabs.append((r, c, _dev(r), _dev(c)))
        ch = np.zeros(case.n, nydus_gpu.CHUNK_DTYPE)
        ch["length"] = case.lengths
        ch["file_index"] = np.arange(case.n)
        rec0 = np.zeros(case.n, nydus_gpu.RESULT_DTYPE)
        rec0["digest"] = case.digests
        rec0["kind"] = DIGESTED
        d_ch = _dev(ch)
        _, _, ref, _ = _dedup(eng, x1, case.digests, case.lengths)  # x1's answer, before any append
        outs, errs, tips = [], [], [x1]
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()

        def prober():
            try:
                for _ in range(40):
                    out = _dev(rec0)
                    torch.cuda.current_stream().synchronize()  # the upload, before the side stream reads it
                    eng.dedup_device(d_ch.data_ptr(), case.n, out.data_ptr(), stream=stream.cuda_stream)
                    outs.append(out)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        def folder():
            try:
                for r, c, d_r, d_c in tabs:
                    tips.append(tips[-1].fold(d_r.data_ptr(), d_c.data_ptr(), 50))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=prober), threading.Thread(target=folder)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        eng.device_status()
        assert len(outs) == 40 and len(tips) == 17
        for out in outs:
            assert out.cpu().numpy().tobytes() == ref.tobytes(), "a dedup against x1 saw a fold"
        assert all(t.info()["shares_base_storage"] for t in tips[1:])
        exp = _appended(R1, nb, _model(seedr, seedc)[0])
        for i, (r, c, _, _) in enumerate(tabs):
            exp = _appended(exp, nb + 1 + i, _model(r, c)[0])
        _same_rows(tips[-1].export()[0], exp, "the tip after 16 folds")
        assert tips[-1].entries == m1 + 16 * 25 and tips[-1].info()["blobs"] == nb + 17
        _, _, after, st = _dedup(eng, tips[-1], case.digests, case.lengths)
        assert after.tobytes() != ref.tobytes()  # the folded digests do turn NEW chunks into DICT ones
        _, _, still, _ = _dedup(eng, x1, case.digests, case.lengths)
        assert still.tobytes() == ref.tobytes()
        eng.set_dict(None)
        for h in tips + [b]:
            h.release()
    finally:
        eng.close()
