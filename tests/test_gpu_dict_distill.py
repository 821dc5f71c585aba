"""Dict distill (ngpu_dict_distill / ngpu_node_dict_distill, csrc/dict.hip +
csrc/dict_distill.hip) on the GPU.

The expectation everywhere is the header's: the first row of every digest that at
least max(min_refs, 1) rows of the base hold, in table order, blobs as the flags
say -- the sequential model of tests/distill_cases.py.  Every case compares the
export (records and blob rows, byte for byte), the info, the count-only info and
the capacities with the model, and the probes of the result with those of a dict
created from the model's rows.

  1  sizes at which a wave, a workgroup, a keep word or a scan tile ends, by
     row pattern; ~70,000 rows so that several workgroups add to one winner
  2  crafted digests: one chain by tag, a chain that wraps, the 0xFFFFFFFF tag
  3  min_refs; a dict of nothing that can be extended
  4  blobs: default, KEEP_BLOBS, MERGE_BLOB_IDS, rows outside the blob count
  5  handles that share a storage; extend, save and open after a distill
  6  a layer processed against base and against distill(base)
  7  node dicts, refusals, the command line
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import distill_cases as ds
import nydus_gpu
from nydus_gpu import rafs
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEEP, MERGE = ds.KEEP_BLOBS, ds.MERGE_BLOB_IDS
CS = 0x10000
T = 256 * 64  # one scan tile: kRetireScanTile keep words of 64 records


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _same_rows(got, exp, tag):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for f in exp.dtype.names if len(exp) else ():
        bad = np.flatnonzero((got[f] != exp[f]).reshape(len(exp), -1).any(axis=1))
        assert not len(bad), f"{tag}: {f} differs in {len(bad)} rows, first {bad[0]}: " \
                             f"got {got[f][bad[0]]}, expected {exp[f][bad[0]]}"
    assert got.tobytes() == exp.tobytes(), tag


def _probe(d, d_q, nq):
    import torch
    hits = torch.zeros(nq * 24, dtype=torch.uint8, device="cuda")
    d.probe_device(d_q.data_ptr(), 32, nq, hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(nydus_gpu.HIT_DTYPE)


def _hits(recs, q):
    return ds.expect_hits(recs, q, nydus_gpu.HIT_DTYPE, nydus_gpu.MISS)


def _queries(rng, recs, extra=()):
    step = max(1, len(recs) // 500)
    return np.concatenate([recs["block_id"][::step], recs["block_id"][-3:], *extra,
                           rng.integers(0, 256, (16, 32), dtype=np.uint8)])


def _check(eng, recs, nb, tbl, min_refs=1, flags=0, tag="", base=None, rng=None, probe=True):
    """distill(base) against the model; -> (out, the model's rows).  base: a handle
    whose rows are recs (default: created here and released)."""
    exp, etbl, einfo = ds.model(recs, nb, tbl, min_refs, flags)
    own = base is None
    if own:
        base = eng.dict_create(recs, tbl)
    kw = {"keep_blobs": bool(flags & KEEP), "merge_blob_ids": bool(flags & MERGE)}
    out, info = base.distill(min_refs, **kw)
    assert info == einfo, (tag, info, einfo)
    none, cinfo = base.distill(min_refs, count_only=True, **kw)
    assert none is None and cinfo == einfo, (tag, cinfo)
    s = len(exp)
    oi = out.info()
    assert (oi["entries"], oi["blobs"]) == (s, einfo["blobs_out"]), (tag, oi)
    assert (oi["record_capacity"], oi["table_capacity"]) == ds.caps(s), (tag, oi)
    assert not oi["shares_base_storage"]
    got, gtbl = out.export()
    _same_rows(got, exp, tag)
    assert gtbl == etbl, tag
    if probe:
        rng = rng or np.random.default_rng(len(recs))
        q = _queries(rng, recs)
        d_q = _dev(q)
        one = eng.dict_create(exp, None if etbl is None else np.frombuffer(etbl, np.uint8))
        if not flags and tbl is not None:
            assert one.info()["blobs"] == oi["blobs"], tag
        want = _hits(exp, q)
        assert _probe(out, d_q, len(q)).tobytes() == want.tobytes(), tag
        assert _probe(one, d_q, len(q)).tobytes() == want.tobytes(), tag
        one.release()
    if own:
        base.release()
    return out, exp


# ---- 1: sizes and row patterns -----------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1]


@pytest.mark.parametrize("m", SIZES)
def test_sizes_and_row_patterns(m):
    rng = np.random.default_rng(3000 + m)
    tbl = ds.table(range(3))
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        for name in ds.PATTERNS:
            recs = ds.pattern(name, rng, m)
            for min_refs in (1, 2) if name in ("triples", "keys", "usize", "dist64") else (1,):
                out, exp = _check(eng, recs, 3, tbl, min_refs, tag=f"m={m} {name} min_refs={min_refs}", rng=rng,
                                  probe=m <= 257 or name in ("one", "keys", "triples"))
                if name == "one" and m:
                    assert len(exp) == 1 and out.entries == 1
                if name == "usize" and m >= 2 and min_refs == 1:
                    # one digest per pair, and the first row's own usize survives
                    assert len(exp) == (m + 1) // 2
                    assert np.array_equal(exp["uncompressed_size"], recs["uncompressed_size"][::2])
                out.release()
        eng.device_status()


def test_several_workgroups_add_to_one_winner():
    """70,001 rows (275 workgroups, 5 scan tiles): one digest in every row; a hot
    digest in every third row among distinct ones; 20 digests all over; whole
    waves of losers; and all distinct."""
    m = 70001
    rng = np.random.default_rng(70)
    tbl = ds.table(range(3))
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        cases = {n: ds.pattern(n, rng, m) for n in ("one", "distinct", "keys", "triples")}
        hot = ds.pattern("distinct", rng, m)
        hot["block_id"][5::3] = hot["block_id"][5]
        cases["hot"] = hot
        few = ds.pattern("distinct", rng, m)
        few["block_id"][100:] = few["block_id"][rng.integers(0, 20, m - 100)]
        cases["few"] = few
        for name, recs in cases.items():
            for min_refs in (1, 3) if name in ("hot", "few") else (1,):
                out, exp = _check(eng, recs, 3, tbl, min_refs, tag=f"{name} min_refs={min_refs}", rng=rng)
                out.release()
        _, _, info = ds.model(cases["one"], 3, tbl)
        assert (info["max_refs"], info["distinct"], info["refs_hist"][16]) == (m, 1, 1)
        eng.device_status()


# ---- 2: crafted digests --------------------------------------------------------------------
def test_crafted_digests_are_counted_apart():
    """Equal home slot and equal tag on unequal digests (none shadows another), a
    chain that wraps the end of the base's table, the 0xFFFFFFFF tag remap, with
    duplicates before and after other members of their chains."""
    rng = np.random.default_rng(0xD157)
    recs, special = ds.crafted(rng)
    tbl = ds.table(range(4))
    win, refs = ds.refs_of(recs)
    assert refs[100] == 4 and refs[300] == 3 and refs[20] == 2 and refs[1500] == 2 and refs[200] == 1
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        base = eng.dict_create(recs, tbl)
        assert base.info()["table_capacity"] == ds.created_table_cap(len(recs))
        q = np.concatenate([recs["block_id"][special], recs["block_id"][::40]])
        d_q = _dev(q)
        for min_refs in (1, 2, 3, 4, 5):
            out, exp = _check(eng, recs, 4, tbl, min_refs, tag=f"crafted min_refs={min_refs}", base=base, rng=rng)
            assert _probe(out, d_q, len(q)).tobytes() == _hits(exp, q).tobytes(), min_refs
            out.release()
        base.release()
        eng.device_status()


# ---- 3: min_refs ---------------------------------------------------------------------------
def test_min_refs_and_a_dict_of_nothing():
    rng = np.random.default_rng(33)
    m = 1000
    recs = ds.rows(rng, m, rng.integers(0, 5, m))
    # refs 1 .. 7: digest j of the first 100 rows is held by 1 + j % 7 rows
    at = 100
    for j in range(100):
        for _ in range(j % 7):
            recs["block_id"][at] = recs["block_id"][j]
            at += 1
    tbl = ds.table(range(5))
    one = ds.pattern("one", rng, 300)
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        base = eng.dict_create(recs, tbl)
        for min_refs in (0, 1, 2, 3, 7, 8, m, m + 1, 0xFFFFFFFF):
            out, exp = _check(eng, recs, 5, tbl, min_refs, tag=f"min_refs={min_refs}", base=base, rng=rng)
            if min_refs <= 1:
                assert out.export()[0].tobytes() == ds.model(recs, 5, tbl, 1)[0].tobytes()
            if min_refs >= 8:
                assert out.entries == 0
            out.release()
        for min_refs, s in ((300, 1), (301, 0), (0xFFFFFFFF, 0)):
            out, exp = _check(eng, one, 3, ds.table(range(3)), min_refs, tag=f"one min_refs={min_refs}", rng=rng)
            assert out.entries == s
            out.release()
        # above every count: 0 entries, 0 blobs, dedups nothing, can be extended
        z, info = base.distill(m + 1)
        assert (z.entries, z.info()["blobs"], z.info()["record_capacity"]) == (0, 0, 0)
        assert (info["entries_out"], info["blobs_out"], info["below_min"]) == (0, 0, info["distinct"])
        q = recs["block_id"][::10]
        d_q = _dev(q)
        assert (_probe(z, d_q, len(q))["entry"] == nydus_gpu.MISS).all()
        assert len(z.export()[0]) == 0 and z.export()[1] is None
        E = ds.rows(rng, 50, 0)
        E["block_id"][:10] = q[:10]
        z1 = z.extend(E, ds.table([77]))
        assert _probe(z1, d_q, len(q)).tobytes() == _hits(E, q).tobytes()
        _same_rows(z1.export()[0], E, "extend of a dict of nothing")
        for h in (z1, z, base):
            h.release()
        eng.device_status()


# ---- 4: blobs ------------------------------------------------------------------------------
def test_blob_rules():
    rng = np.random.default_rng(44)
    m, nb = 2000, 9
    # blobs 0..8: 3 is left empty by the distill (all its rows are shadows), 8 (the
    # last) too; 5 never had a row; 6 only holds rows below min_refs 2
    recs = ds.rows(rng, m, rng.choice([0, 1, 2, 4, 7], m))
    recs["blob_index"][:5] = (0, 1, 2, 4, 7)
    for b, lo in ((3, 600), (8, 700)):
        recs["blob_index"][lo:lo + 50] = b
        recs["block_id"][lo:lo + 50] = recs["block_id"][lo - 500:lo - 450]
    recs["blob_index"][900:920] = 6
    recs["block_id"][1000:1400] = recs["block_id"][200:600]  # refs 2 (and 3 where blob 3 / 8 repeat them)
    tbl = ds.table(range(nb))
    # ids repeat: blobs 0, 2, 7 are one id; 3 and 4 another; 5 and 8 a third (both dead)
    ids = [10, 11, 10, 12, 12, 13, 14, 10, 13]
    rtbl = ds.table(ids)
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        for t, name in ((tbl, "table"), (None, "count")):
            base = eng.dict_create(recs, t)
            if t is None:
                assert base.info()["blobs"] == nb  # blob 8 has rows; 5 lies inside the count
            for min_refs in (1, 2):
                for flags in (0, KEEP):
                    out, exp = _check(eng, recs, nb, t, min_refs, flags, f"{name} min_refs={min_refs} flags={flags}",
                                      base=base, rng=rng)
                    if flags == 0:
                        assert out.info()["blobs"] == (5 if min_refs == 2 else 6), (name, min_refs)
                    else:
                        assert out.info()["blobs"] == nb
                        assert set(int(b) for b in exp["blob_index"]) <= {0, 1, 2, 4, 6, 7}
                    out.release()
            base.release()
        # MERGE_BLOB_IDS on a table that repeats ids
        base = eng.dict_create(recs, rtbl)
        for min_refs in (1, 2):
            out, exp = _check(eng, recs, nb, rtbl, min_refs, MERGE, f"merge min_refs={min_refs}", base=base, rng=rng)
            got_ids = [x.decode() for x in np.frombuffer(out.export()[1], rafs.BLOB_DTYPE)["blob_id"]]
            assert got_ids == [f"{i:064x}" for i in ((10, 11, 12) if min_refs == 2 else (10, 11, 12, 14))]
            # the row kept is the earliest of its id: blob 3's for id 12, though only blob 4 has survivors
            assert out.export()[1][2 * 256:3 * 256] == rtbl[3].tobytes()
            out.release()
        # without a table there is nothing to merge by: refused, *out NULL, info zeroed
        bare = eng.dict_create(recs)
        h, info = ctypes.c_void_p(0xDEAD), nydus_gpu.NgpuDictDistillInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
        rc = nydus_gpu.lib().ngpu_dict_distill(eng._h, bare._h, 1, MERGE, ctypes.byref(h), ctypes.byref(info))
        assert rc == nydus_gpu.EINVAL and h.value is None and bytes(info) == bytes(312)
        bare.release()
        base.release()
        eng.device_status()


def test_rows_outside_the_blob_count_and_no_placements():
    """ngpu_dict_create_device takes the caller's word for n_blobs: rows whose blob
    is >= blobs(base) are kept as they are and make no blob live.  Such a dict
    keeps no placements, and neither does the result."""
    rng = np.random.default_rng(45)
    m = 700
    recs = ds.rows(rng, m, rng.choice([0, 2, 3, 5, 9], m))
    recs["block_id"][300:500] = recs["block_id"][:200]
    recs["blob_index"][:200] = rng.choice([2, 9], 200)  # blobs 0 and 3 keep rows among the rest
    recs["uncompressed_offset"] = 0
    recs["compressed_offset"], recs["flags"] = 0, 0
    recs["compressed_size"] = recs["uncompressed_size"]  # what a dict without placements exports
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        dv = [_dev(np.ascontiguousarray(recs[f])) for f in ("block_id", "uncompressed_size", "blob_index", "index")]
        base = eng.dict_create_device(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), m,
                                      n_blobs=4)
        _same_rows(base.export()[0], recs, "base")
        for flags in (0, KEEP):
            out, exp = _check(eng, recs, 4, None, 1, flags, f"outside flags={flags}", base=base, rng=rng, probe=False)
            # blob 1 never had a row: 0, 2, 3 -> 0, 1, 2; 5 and 9 stay 5 and 9
            assert sorted(set(int(b) for b in exp["blob_index"])) == ([0, 1, 2, 5, 9] if not flags else [0, 2, 3, 5, 9])
            assert out.info()["blobs"] == (3 if not flags else 4)
            out.release()
        base.release()
        eng.device_status()


# ---- 5: handles ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layer(oracle):
    """A layer of ~100 chunks with intra-layer duplicates, and its digests."""
    rng = np.random.default_rng(50)
    total = 4 << 20
    data = bytearray(rng.integers(0, 256, total, dtype=np.uint8).tobytes())
    chunks, off = [], 0
    while True:
        ln = int(rng.integers(1, CS + 1)) if rng.random() < 0.5 else CS
        if off + ln > total:
            break
        chunks.append((off, ln, len(chunks), 0))
        off = (off + ln + 511) // 512 * 512
    ch = np.array(chunks, dtype=nydus_gpu.CHUNK_DTYPE)
    for a, b in ((3, 40), (3, 41), (10, 70)):
        ch["length"][b] = ch["length"][a]
        data[ch["offset"][b]:ch["offset"][b] + ch["length"][a]] = data[ch["offset"][a]:ch["offset"][a] + ch["length"][a]]
    data = bytes(data)
    dig = oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), "blake3")
    return data, ch, dig


def _layer_rows(rng, layer, blobs):
    _, ch, dig = layer
    r = ds.rows(rng, len(ch), blobs)
    r["block_id"], r["uncompressed_size"] = dig, ch["length"]
    return r


def test_handles_on_a_shared_storage(layer):
    """d0 = create(A), d1 = extend(d0, B) (a fork), d2 = extend(d1, C) in place, C
    repeating digests of A and B: distill(d1) is the model over A ++ B and blind to
    C's slots and rows, distill(d2) the model over all three; d1 and d2 export and
    answer a process as before."""
    rng = np.random.default_rng(51)
    data, ch, dig = layer
    A = np.concatenate([ds.rows(rng, 500, rng.integers(0, 2, 500)), _layer_rows(rng, layer, 1)])
    A["blob_index"][:2] = (0, 1)
    B = ds.rows(rng, 400, rng.integers(0, 2, 400))
    B["blob_index"][:2] = (0, 1)
    B["block_id"][100:200] = A["block_id"][:100]
    C = ds.rows(rng, 300, 0)
    C["block_id"][:100] = A["block_id"][200:300]
    C["block_id"][100:150] = B["block_id"][300:350]
    C["block_id"][150:200] = C["block_id"][200:250]
    C["block_id"][250:250 + 30] = dig[:30]
    ta, tb, tc = ds.table([1, 2]), ds.table([3, 4]), ds.table([5])
    AB = np.concatenate([A, B])
    AB["blob_index"][len(A):] += 2
    ABC = np.concatenate([AB, C])
    ABC["blob_index"][len(AB):] += 4
    tab, tabc = np.concatenate([ta, tb]), np.concatenate([ta, tb, tc])
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        d0 = eng.dict_create(A, ta)
        d1 = d0.extend(B, tb)
        assert not d1.info()["shares_base_storage"]
        before1 = (d1.export(), eng.process(data, ch, dict=d1))
        assert before1[1][1]["dict_chunks"] > 0
        o1, e1 = _check(eng, AB, 4, tab, 1, tag="d1", base=d1, rng=rng)
        d2 = d1.extend(C, tc)
        assert d2.info()["shares_base_storage"]
        before2 = (d2.export(), eng.process(data, ch, dict=d2))
        # d1 again, with C's rows and slots on its storage
        o1b, _ = _check(eng, AB, 4, tab, 1, tag="d1 after the in-place extend", base=d1, rng=rng)
        assert o1b.export()[0].tobytes() == o1.export()[0].tobytes()
        for min_refs in (1, 2):
            o, _ = _check(eng, AB, 4, tab, min_refs, tag=f"d1 min_refs={min_refs}", base=d1, rng=rng)
            o.release()
            o, _ = _check(eng, ABC, 5, tabc, min_refs, tag=f"d2 min_refs={min_refs}", base=d2, rng=rng)
            o.release()
        _same_rows(d0.export()[0], A, "d0")
        for d, (exp0, (res0, st0)) in ((d1, before1), (d2, before2)):
            got = d.export()
            assert got[0].tobytes() == exp0[0].tobytes() and got[1] == exp0[1]
            res, st = eng.process(data, ch, dict=d)
            assert res.tobytes() == res0.tobytes() and st == st0
        for h in (o1b, o1, d2, d1, d0):
            h.release()
        eng.device_status()


def test_extend_save_and_open_after_a_distill(tmp_path):
    rng = np.random.default_rng(52)
    m = 3000
    recs = ds.pattern("triples", rng, m)
    tbl = ds.table(range(3))
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        out, exp = _check(eng, recs, 3, tbl, 1, tag="base", rng=rng)
        s = out.entries
        cap, tcap = ds.caps(s)
        E = ds.rows(rng, s // 2, 0)
        E["block_id"][:20] = exp["block_id"][:20]  # the survivors' rows win
        e1 = out.extend(E, ds.table([9]))
        ie = e1.info()
        assert (ie["record_capacity"], ie["table_capacity"], ie["shares_base_storage"]) == (cap, tcap, True)
        rows = np.concatenate([exp, E])
        rows["blob_index"][s:] += 3
        q = np.concatenate([recs["block_id"][::7], E["block_id"]])
        d_q = _dev(q)
        assert _probe(e1, d_q, len(q)).tobytes() == _hits(rows, q).tobytes()
        assert _probe(out, d_q, len(q)).tobytes() == _hits(exp, q).tobytes()  # out is blind to it
        # a distill of the extended dict drops the 20 shadows again
        o2, _ = _check(eng, rows, 4, np.concatenate([tbl, ds.table([9])]), 1, tag="again", base=e1, rng=rng)
        assert o2.entries == s + len(E) - 20
        # save, then open: the same export
        path = str(tmp_path / "distilled.boot")
        info = out.save(path)
        assert info["entries"] == s
        back = eng.dict_open(path)
        got, gtbl = back.export()
        want, wtbl = out.export()
        assert got.tobytes() == want.tobytes() and gtbl == wtbl
        for h in (back, o2, e1, out):
            h.release()
        eng.device_status()


# ---- 6: end to end -------------------------------------------------------------------------
def test_a_layer_against_base_and_against_its_distill(layer):
    """Every digest answers as in base: kind, digest, chunk index, uncompressed
    offset and the blob id are equal chunk for chunk; ref and the inner blob index
    go through the renumbering.  Count only leaves the engine's counters alone."""
    rng = np.random.default_rng(60)
    data, ch, dig = layer
    n = len(ch)
    # the layer's digests three times over in blobs 1, 3, 4, among filler; blob 2 only holds shadows
    first = _layer_rows(rng, layer, 1)
    first["uncompressed_size"][::7] = 0
    recs = np.concatenate([ds.rows(rng, 300, 0), first[:n // 2], ds.rows(rng, 200, rng.integers(0, 2, 200)),
                           _layer_rows(rng, layer, 2)[:n // 2], _layer_rows(rng, layer, 3),
                           _layer_rows(rng, layer, 4), ds.rows(rng, 100, 4)])
    nb = 5
    tbl = ds.table(range(100, 100 + nb))
    ids = [x.decode() for x in np.frombuffer(tbl.tobytes(), rafs.BLOB_DTYPE)["blob_id"]]
    with nydus_gpu.Engine(chunk_size=CS) as eng:
        base = eng.dict_create(recs, tbl)
        c0 = eng.counters()
        _, cinfo = base.distill(1, count_only=True)
        assert eng.counters() == c0
        out, exp = _check(eng, recs, nb, tbl, 1, tag="layer", base=base, rng=rng)
        assert cinfo["entries_out"] == out.entries and cinfo["shadowed"] >= n
        assert out.info()["blobs"] == 4  # blob 2 left
        oids = [x.decode() for x in np.frombuffer(out.export()[1], rafs.BLOB_DTYPE)["blob_id"]]
        assert oids == ids[:2] + ids[3:]
        rb, sb = eng.process(data, ch, dict=base)
        ro, so = eng.process(data, ch, dict=out)
        one = eng.dict_create(exp, np.frombuffer(out.export()[1], np.uint8))
        r1, s1 = eng.process(data, ch, dict=one)
        assert ro.tobytes() == r1.tobytes() and so == s1
        hit = rb["kind"] == nydus_gpu.DICT
        assert hit.sum() >= n // 2 and np.array_equal(ro["digest"], dig)
        for f in ("kind", "digest", "index", "uncompressed_offset"):
            assert np.array_equal(rb[f], ro[f]), f
        assert [ids[int(b)] for b in rb["dict_blob"][hit]] == [oids[int(b)] for b in ro["dict_blob"][hit]]
        # the renumbering: entry ids are positions among the survivors
        win, _ = ds.refs_of(recs)
        newid = np.cumsum(win == np.arange(len(recs))) - 1
        assert np.array_equal(ro["ref"][hit], newid[rb["ref"][hit].astype(np.int64)].astype(np.uint64))
        for f in ("chunks", "new_chunks", "intra_chunks", "dict_chunks", "new_bytes"):
            assert sb[f] == so[f], f
        for h in (one, out, base):
            h.release()
        eng.device_status()


# ---- 7: nodes, refusals, the command line ----------------------------------------------------
def test_node_dicts(layer):
    import torch
    rng = np.random.default_rng(70)
    data, ch, dig = layer
    n = len(ch)
    recs = np.concatenate([ds.rows(rng, 400, rng.integers(0, 3, 400)), _layer_rows(rng, layer, 1)[:n // 2],
                           _layer_rows(rng, layer, 3), _layer_rows(rng, layer, 2)])
    recs["block_id"][100:200] = recs["block_id"][:100]
    nb = 4
    tbl = ds.table(range(nb))
    d_data, d_ch = _dev(np.frombuffer(data, np.uint8)), _dev(ch)

    def run(node, i, d):
        out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        node.process_device(i, d, d_data.data_ptr(), d_data.numel(), d_ch.data_ptr(), n, out.data_ptr(),
                            stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)

    node = nydus_gpu.Node([0, 0], chunk_size=CS)
    try:
        d = node.dict_create(recs, tbl, mode=nydus_gpu.NODE_DICT_REPLICATE)
        with nydus_gpu.Engine(chunk_size=CS) as eng:
            plain = eng.dict_create(recs, tbl)
            for min_refs in (1, 2):
                exp, etbl, einfo = ds.model(recs, nb, tbl, min_refs)
                r, info = node.dict_distill(d, min_refs)
                assert info == einfo and node.dict_distill(d, min_refs, count_only=True) == (None, einfo)
                assert (r.entries, r.info()["blobs"]) == (len(exp), einfo["blobs_out"])
                assert r.info()["record_capacity"] == ds.caps(len(exp))[0]
                got, gtbl = node.dict_export(r)
                _same_rows(got, exp, f"node export min_refs={min_refs}")
                assert gtbl == etbl
                pr, pinfo = plain.distill(min_refs)
                assert pinfo == info and pr.export()[0].tobytes() == got.tobytes()
                o = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
                eng.process_dict_device(pr, d_data.data_ptr(), d_data.numel(), d_ch.data_ptr(), n, o.data_ptr())
                torch.cuda.synchronize()
                want = o.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
                assert (want["kind"] == nydus_gpu.DICT).sum() > 0
                for part in range(2):
                    assert run(node, part, r).tobytes() == want.tobytes(), (min_refs, part)
                if min_refs == 1:  # a distilled node dict can be extended, in place
                    x1 = node.dict_extend(r, recs[:40], tbl)
                    assert x1.info()["shares_base_storage"] and x1.entries == len(exp) + 40
                    x1.release()
                pr.release()
                r.release()
            _same_rows(node.dict_export(d)[0], recs, "node base export")
            # a plain dict is not for the node call, a node dict not for the engine call
            L = nydus_gpu.lib()
            for fn, a, b in ((L.ngpu_node_dict_distill, node._h, plain._h), (L.ngpu_dict_distill, eng._h, d._h)):
                h, info = ctypes.c_void_p(0xDEAD), nydus_gpu.NgpuDictDistillInfo()
                ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
                assert fn(a, b, 1, 0, ctypes.byref(h), ctypes.byref(info)) == nydus_gpu.EINVAL
                assert h.value is None and bytes(info) == bytes(312)
            plain.release()
        # partitioned: NGPU_EUNSUPP, *out NULL, info zeroed, the base still usable
        p = node.dict_create(recs, tbl, mode=nydus_gpu.NODE_DICT_PARTITION)
        h, info = ctypes.c_void_p(0xDEAD), nydus_gpu.NgpuDictDistillInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
        rc = nydus_gpu.lib().ngpu_node_dict_distill(node._h, p._h, 1, 0, ctypes.byref(h), ctypes.byref(info))
        assert rc == nydus_gpu.EUNSUPP and h.value is None and bytes(info) == bytes(312)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            node.dict_distill(p, 1, count_only=True)
        assert x.value.code == nydus_gpu.EUNSUPP
        assert run(node, 0, p).tobytes() == run(node, 1, d).tobytes()
        for hnd in (p, d):
            hnd.release()
    finally:
        node.close()


def test_inspect_distill_save_dict(tmp_path):
    """inspect --dict A --dict A --distill --save-dict OUT: OUT reopens with the
    entries of A alone, and the report's distill.shadowed is entries(A)."""
    rng = np.random.default_rng(80)
    a_rows = ds.rows(rng, 500, rng.integers(0, 2, 500), 0x100000)
    a_rows["blob_index"][:2] = (0, 1)
    cs = 0x100000
    a = tmp_path / "a.boot"
    a.write_bytes(rafs.write_v6_bootstrap(a_rows, cs, flags=0x5, blobs=rafs.make_blob_table(["ab" * 32, "cd" * 32], cs)))
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "nydus-snapshotter_amd")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    outp = tmp_path / "out.boot"
    r = subprocess.run([sys.executable, "-m", "nydus_gpu.inspect", "--dict", str(a), "--dict", str(a), "--distill",
                        "--save-dict", str(outp)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = json.loads(r.stdout)
    assert rep["distill"]["shadowed"] == 500 and rep["distill"]["entries_in"] == 1000
    assert (rep["distill"]["blobs_in"], rep["distill"]["blobs_out"], rep["distill"]["max_refs"]) == (4, 2, 2)
    assert (rep["entries"], rep["blobs"]) == (500, 2)
    with nydus_gpu.Engine(chunk_size=cs) as eng:
        want, got = eng.dict_open(str(a)), eng.dict_open(str(outp))
        assert got.entries == 500
        w, g = want.export(), got.export()
        assert g[0].tobytes() == w[0].tobytes() and g[1] == w[1]
        # --merge-blob-ids implies a distill; with it the two copies' blobs are one again either way
        from nydus_gpu import inspect as ins
        rep2 = ins.save_dict(str(tmp_path / "out2.boot"), [str(a), str(a)], merge_blob_ids=True)
        assert rep2["distill"]["blobs_out"] == 2 and rep2["entries"] == 500
        want.release()
        got.release()
