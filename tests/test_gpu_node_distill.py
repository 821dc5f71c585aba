"""Distill of node dicts across their parts (ngpu_node_dict_distill_parts,
csrc/node.hip + csrc/node_distill.hip) on the GPU, on nodes that list device 0 W
times.

The expectation everywhere is the header's: the first row of every digest, in
global table order, that at least max(min_refs, 1) rows of the base hold, blobs as
the flags say -- the sequential model of tests/distill_cases.py over the whole
dict, whatever W is.  Every case holds the result to all of these: (a) the export
equals the model's rows and blob table byte for byte; (b) probes through every
engine of the node (a node dict is probed through an engine: set_dict and a dedup
call, every result field and every stats field) equal distill_cases.expect_hits
over the model's rows and the same call on a plain Engine against its
ChunkDict.distill of the same rows, whose own hits equal expect_hits byte for
byte; (c) the info and the count-only info equal the model's; (d) the export of
the base is unchanged.  Rows are placed on owners by their first two digest bytes
(every row of a digest alike).

  1  sizes at which a wave, a workgroup's run of tiles or a keep word ends, by row
     pattern; W in 2, 3, 5, 8 and both exchanges
  2  the gid bit fold: one part owns every row, one part owns none, kept rows
     alone in their 32-bit words, and owners that alternate every row
  3  blobs across parts under each flag; 63 / 64 / 65 blobs; a blob count alone
  4  min_refs, a dict of nothing that can be extended
  5  node_cases' crafted part tables with duplicates before and after
  6  handles: older handles, growth in place after a distill, save and open,
     placement rows
  7  real layers: Node.process_step and a streaming Node.pack against the result
  8  refusals, and the old call's answers next to the new one
"""
import ctypes

import numpy as np
import pytest

import dedup_cases as dc
import distill_cases as ds
import node_cases as nc
import nydus_gpu
from nydus_gpu import rafs
from test_gpu_dict_fold import _appended, _dev, _places, _tables
from test_gpu_dict_retire import _same_rows
from test_gpu_node_fold import MODES, _agree, _ask, _k_of, _nfold, _node_model

pytestmark = pytest.mark.gpu

KEEP, MERGE = ds.KEEP_BLOBS, ds.MERGE_BLOB_IDS
CS = 0x10000


@pytest.fixture(scope="module")
def node_of():
    """One Node per W, reused by every case that asks for it; the previous one is
    closed when another is asked for."""
    held = {}

    def get(W):
        if W not in held:
            for n in held.values():
                n.close()
            held.clear()
            held[W] = nydus_gpu.Node([0] * W, chunk_size=CS, staging_bytes=4 * CS)
        return held[W]

    yield get
    for n in held.values():
        n.close()


@pytest.fixture(scope="module")
def plain():
    eng = nydus_gpu.Engine(chunk_size=CS, staging_bytes=4 * CS)
    yield eng
    eng.close()


def _place(rng, recs, W, owners=None):
    """Digest prefixes (the first 16 bits) drawn from an owner's range, every row of
    a digest alike.  owners: one per row, the first row of a digest decides
    (default: random).  -> the rows' owners."""
    m = len(recs)
    if not m:
        return np.zeros(0, np.int64)
    win, _ = ds.refs_of(recs)
    o = (rng.integers(0, W, m) if owners is None else np.asarray(owners, np.int64))[win]
    lo, hi = -(-o * 65536 // W), -(-(o + 1) * 65536 // W) - 1
    p = rng.integers(lo, hi + 1)[win]
    recs["block_id"][:, 0] = p >> 8
    recs["block_id"][:, 1] = p & 0xFF
    assert (dc.owner_of(recs["block_id"], W) == o).all()
    win2, _ = ds.refs_of(recs)
    assert np.array_equal(win, win2)  # the prefixes made no two digests equal
    return o


def _hits(recs, q):
    return ds.expect_hits(recs, q, nydus_gpu.HIT_DTYPE, nydus_gpu.MISS)


def _once(q):
    """Every digest of q once, in order: a digest asked twice is an INTRA chunk of
    the dedup call."""
    return np.ascontiguousarray(np.stack([np.frombuffer(b, np.uint8) for b in dict.fromkeys(bytes(x) for x in q)]))


def _queries(rng, recs, extra=()):
    """Digests of the rows (a sample), the extra ones and fresh misses, each once."""
    step = max(1, len(recs) // 400)
    return _once(np.concatenate([recs["block_id"][::step], recs["block_id"][-3:], *extra,
                                 rng.integers(0, 256, (16, 32), dtype=np.uint8)]))


def _probe(d, d_q, nq):
    """ngpu_dict_hit rows of nq digests against a plain dict."""
    import torch
    hits = torch.zeros(nq * 24, dtype=torch.uint8, device="cuda")
    d.probe_device(d_q.data_ptr(), 32, nq, hits.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(nydus_gpu.HIT_DTYPE)


def _lens(want):
    """Chunk lengths at which every row that holds a query's digest answers it."""
    return np.where((want["entry"] != nydus_gpu.MISS) & (want["usize"] != 0), want["usize"], CS).astype(np.uint32)


def _node_answers(tag, node, d, rows, q, ref=None):
    """Every engine of the node answers the (distinct) digests q against d as
    expect_hits over `rows` says, and as `ref` (an _ask of the same call elsewhere)."""
    want = _hits(rows, q)
    lens = _lens(want)
    hit = want["entry"] != nydus_gpu.MISS
    for i, e in enumerate(node.engines):
        try:
            host, st = _ask(e, d, q, lens)
        finally:
            e.set_dict(None)
        assert np.array_equal(host["kind"] == nydus_gpu.DICT, hit), (tag, i)
        for f, g in (("ref", "entry"), ("index", "index"), ("dict_blob", "blob"),
                     ("uncompressed_offset", "uncompressed_offset")):
            assert np.array_equal(host[f][hit], want[g][hit].astype(host[f].dtype)), (tag, i, f)
        if ref is not None:
            _agree(f"{tag} engine {i}", (host, st), ref)


def _export_equals(tag, node, d, rows, tbl):
    got, gtbl = node.dict_export_parts(d)
    _same_rows(got, rows, tag)
    if tbl is not None and not isinstance(tbl, bytes):
        tbl = np.ascontiguousarray(tbl).tobytes()
    assert gtbl == tbl, tag
    return got, gtbl


def _kw(flags):
    return {"keep_blobs": bool(flags & KEEP), "merge_blob_ids": bool(flags & MERGE)}


def _check(node, plain, recs, nb, tbl, mode="copy", min_refs=1, flags=0, tag="", base=None, rng=None, q=None,
           probe=True):
    """distill_parts(base) against the model, (a) to (d); -> (out, the model's rows).
    base: a handle of this node whose rows are recs (default: created here and
    released)."""
    W = len(node.engines)
    exp, etbl, einfo = ds.model(recs, nb, tbl, min_refs, flags)
    own = base is None
    if own:
        base = node.dict_create(recs, tbl, mode=MODES[mode])
    binfo = base.info()
    out, info = node.dict_distill_parts(base, min_refs, **_kw(flags))
    assert info == einfo, (tag, info, einfo)                                       # (c)
    none, cinfo = node.dict_distill_parts(base, min_refs, count_only=True, **_kw(flags))
    assert none is None and cinfo == einfo, (tag, cinfo, einfo)
    s = len(exp)
    oi = out.info()
    assert (oi["entries"], oi["blobs"]) == (s, einfo["blobs_out"]), (tag, oi)
    if mode != "replicate":  # part 0's storage: a retire's room for its own survivors
        s0 = int((dc.owner_of(exp["block_id"], W) == 0).sum()) if s else 0
        assert (oi["record_capacity"], oi["table_capacity"]) == ds.caps(s0), (tag, oi, s0)
    assert not oi["shares_base_storage"], tag
    got, _ = _export_equals(tag, node, out, exp, etbl)                             # (a)
    if probe:                                                                      # (b)
        rng = rng or np.random.default_rng(len(recs))
        q = _queries(rng, recs) if q is None else _once(q)
        want = _hits(exp, q)
        pd = plain.dict_create(recs, tbl)
        pr, pinfo = pd.distill(min_refs, **_kw(flags))
        assert pinfo == info, (tag, pinfo)
        assert _probe(pr, _dev(q), len(q)).tobytes() == want.tobytes(), tag
        pgot, ptbl = pr.export()
        assert pgot.tobytes() == got.tobytes() and ptbl == etbl, tag
        try:
            ref = _ask(plain, pr, q, _lens(want))
        finally:
            plain.set_dict(None)
        _node_answers(tag, node, out, exp, q, ref)
        pr.release()
        pd.release()
    assert base.info() == binfo, tag                                               # (d)
    _export_equals(tag + " base", node, base, recs, tbl)
    if own:
        base.release()
    return out, exp


# ---- 1: sizes and row patterns -----------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 4097]


@pytest.mark.parametrize("m", SIZES)
def test_sizes_and_row_patterns(m, node_of, plain):
    """W = 2, the copy exchange.  4097 rows give a part two workgroups of four-tile
    runs: the counters in LDS and the wave's last blob are carried over tiles."""
    node = node_of(2)
    rng = np.random.default_rng(9000 + m)
    tbl = ds.table(range(3))
    for name in ds.PATTERNS:
        recs = ds.pattern(name, rng, m)
        _place(rng, recs, 2)
        for min_refs in (1, 2) if name in ("triples", "keys", "usize", "dist64") else (1,):
            out, exp = _check(node, plain, recs, 3, tbl, "copy", min_refs, tag=f"m={m} {name} min_refs={min_refs}",
                              rng=rng, probe=m <= 257 or name in ("one", "keys", "triples"))
            if name == "one" and m:
                assert len(exp) == 1 and out.entries == 1
            out.release()
    for e in node.engines:
        e.device_status()


@pytest.mark.parametrize("mode", ["copy", "routed"])
@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_parts_and_exchanges(W, mode, node_of, plain):
    node = node_of(W)
    rng = np.random.default_rng(9100 + 10 * W + (mode == "routed"))
    m = 4097
    tbl = ds.table(range(3))
    for name in ("triples", "keys", "one"):
        recs = ds.pattern(name, rng, m)
        _place(rng, recs, W)
        for min_refs in (1, 2) if name != "one" else (1,):
            out, _ = _check(node, plain, recs, 3, tbl, mode, min_refs, tag=f"W={W} {mode} {name} min_refs={min_refs}",
                            rng=rng)
            out.release()
    for e in node.engines:
        e.device_status()


# ---- 2: the gid bit fold -----------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one_owner", "one_empty", "alone_in_a_word", "alternate"])
def test_gid_bit_fold(layout, node_of, plain):
    """W = 3, 2048 rows.  one_owner: every row on part 2, so whole waves share two
    32-bit words of the bitmap and the runs are 32 lanes long; one_empty: part 1 has
    no row; alone_in_a_word: groups of 32 rows of one digest, the groups' owners
    alternating, so every kept row is the only one of its part in its 32-bit word
    and every run is one kept row; alternate: distinct rows whose owner steps with
    every row."""
    W, m = 3, 2048
    node = node_of(W)
    rng = np.random.default_rng(9200 + len(layout))
    tbl = ds.table(range(3))
    if layout == "alone_in_a_word":
        recs = ds.pattern("distinct", rng, m)
        recs["block_id"] = np.repeat(recs["block_id"][::32], 32, axis=0)
        owners = (np.arange(m) // 32) % W
    elif layout == "alternate":
        recs = ds.pattern("distinct", rng, m)
        owners = np.arange(m) % W
    else:
        recs = ds.pattern("triples", rng, m)
        if layout == "one_owner":
            owners = np.full(m, W - 1)
        else:
            owners = rng.integers(0, W - 1, m)
            owners[owners >= W // 2] += 1
    own = _place(rng, recs, W, owners)
    pm = np.bincount(own, minlength=W)
    if layout == "one_owner":
        assert list(pm) == [0, 0, m]
    if layout == "one_empty":
        assert pm[1] == 0 and pm[0] and pm[2]
    for mode in ("copy", "routed"):
        for min_refs in (1, 2, 3) if layout in ("one_owner", "one_empty") else (1, 32, 33):
            out, exp = _check(node, plain, recs, 3, tbl, mode, min_refs, tag=f"{layout} {mode} min_refs={min_refs}",
                              rng=rng)
            if layout == "alone_in_a_word":
                assert len(exp) == (m // 32 if min_refs <= 32 else 0)
            out.release()
    for e in node.engines:
        e.device_status()


# ---- 3: blobs across parts ---------------------------------------------------------------
def _blob_case(rng):
    """512 rows, 9 blobs, W = 2.  Blob 5's only survivors are on part 1; blob 3 has
    rows only on part 0, all of them shadows (it leaves); blob 7 has no row at all;
    blob 1's survivors are all on part 0 and blob 6's all on part 1 (the repeated
    table gives the two one id); the rest is spread."""
    m = 512
    recs = ds.rows(rng, m, rng.choice([0, 2, 4, 8], m))
    recs["blob_index"][:4] = (0, 2, 4, 8)
    owners = rng.integers(0, 2, m)
    for b, lo, o in ((5, 100, 1), (1, 140, 0), (6, 180, 1)):
        recs["blob_index"][lo:lo + 30] = b
        owners[lo:lo + 30] = o
    owners[20:60] = 0
    recs["blob_index"][300:340] = 3
    recs["block_id"][300:340] = recs["block_id"][20:60]  # shadows of part 0's rows
    recs["block_id"][400:430] = recs["block_id"][100:130]  # blob 5's digests again, in blob 0
    recs["blob_index"][400:430] = 0
    own = _place(rng, recs, 2, owners)
    exp, _, _ = ds.model(recs, 9, None, 1, KEEP)  # (KEEP_BLOBS: the rows keep their blob indices)
    eo = dc.owner_of(exp["block_id"], 2)
    assert set(eo[exp["blob_index"] == 5]) == {1} and set(eo[exp["blob_index"] == 1]) == {0}
    assert set(eo[exp["blob_index"] == 6]) == {1} and not (exp["blob_index"] == 3).any()
    assert set(own[recs["blob_index"] == 3]) == {0} and not (recs["blob_index"] == 7).any()
    return recs


def test_blobs_across_parts(node_of, plain):
    node = node_of(2)
    rng = np.random.default_rng(9300)
    recs = _blob_case(rng)
    nb = 9
    tbl = ds.table(range(nb))
    rtbl = ds.table([10, 11, 12, 13, 14, 15, 11, 16, 17])  # blobs 1 and 6 are one id
    for t, name in ((tbl, "table"), (None, "count")):
        base = node.dict_create(recs, t, mode=MODES["copy"])
        assert base.info()["blobs"] == nb
        for min_refs in (1, 2):
            for flags in (0, KEEP):
                out, exp = _check(node, plain, recs, nb, t, "copy", min_refs, flags,
                                  f"{name} min_refs={min_refs} flags={flags}", base=base, rng=rng)
                if flags == KEEP:
                    assert out.info()["blobs"] == nb
                elif min_refs == 1:  # 3 and 7 leave; 5 stays though part 0 has no survivor in it
                    assert out.info()["blobs"] == 7
                    assert sorted(set(int(b) for b in exp["blob_index"])) == list(range(7))
                else:                # only blob 5's digests (and blob 3's winners) are held twice
                    assert out.info()["blobs"] < 7
                out.release()
        base.release()
    base = node.dict_create(recs, rtbl, mode=MODES["copy"])
    for mode_flags, blobs in ((MERGE, 6), (0, 7)):
        out, exp = _check(node, plain, recs, nb, rtbl, "copy", 1, mode_flags, f"repeated ids flags={mode_flags}",
                          base=base, rng=rng)
        assert out.info()["blobs"] == blobs
        if mode_flags == MERGE:  # the two blobs of one id, survivors on different parts, are one row
            ids = [x.decode() for x in np.frombuffer(node.dict_export_parts(out)[1], rafs.BLOB_DTYPE)["blob_id"]]
            assert ids == [f"{i:064x}" for i in (10, 11, 12, 14, 15, 17)]
        out.release()
    base.release()
    # MERGE_BLOB_IDS without a blob table: refused, *out NULL, info zeroed
    bare = node.dict_create(recs, mode=MODES["copy"])
    h, info = ctypes.c_void_p(0xDEAD), nydus_gpu.NgpuDictDistillInfo()
    ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
    rc = nydus_gpu.lib().ngpu_node_dict_distill_parts(node._h, bare._h, 1, MERGE, ctypes.byref(h), ctypes.byref(info))
    assert rc == nydus_gpu.EINVAL and h.value is None and bytes(info) == bytes(312)
    bare.release()
    for e in node.engines:
        e.device_status()


@pytest.mark.parametrize("nb", [63, 64, 65])
def test_blob_counts_with_a_table(nb, node_of, plain):
    """Every blob has a winner; the odd blobs' digests are all held twice, so
    min_refs = 2 keeps the odd blobs and drops the even ones, the last word of the
    live bitmap included."""
    node = node_of(2)
    rng = np.random.default_rng(9400 + nb)
    m = 4 * nb
    recs = ds.rows(rng, m, 0)
    recs["blob_index"][:2 * nb] = np.arange(2 * nb) // 2
    recs["blob_index"][2 * nb:] = nb - 1
    odd = np.flatnonzero(recs["blob_index"][:2 * nb] % 2 == 1)
    recs["block_id"][2 * nb:2 * nb + len(odd)] = recs["block_id"][odd]
    _place(rng, recs, 2)
    tbl = ds.table(range(nb))
    base = node.dict_create(recs, tbl, mode=MODES["copy"])
    for min_refs, flags in ((1, 0), (2, 0), (2, KEEP), (2, MERGE)):
        out, exp = _check(node, plain, recs, nb, tbl, "copy", min_refs, flags, f"nb={nb} {min_refs} {flags}",
                          base=base, rng=rng)
        assert out.info()["blobs"] == (nb if min_refs == 1 or flags == KEEP else nb // 2)
        out.release()
    base.release()


# ---- 4: min_refs -------------------------------------------------------------------------
def test_min_refs_and_a_dict_of_nothing(node_of, plain):
    """Triples whose digests all belong to part 0 among single rows of part 1 (and a
    digest on 7 rows of part 1): min_refs = 3 keeps part 0's triples while part 1
    keeps one row, min_refs = 4 .. 7 leave part 0 with nothing."""
    node = node_of(2)
    rng = np.random.default_rng(9500)
    m = 1500
    recs = ds.pattern("triples", rng, 900)
    recs = np.concatenate([recs, ds.rows(rng, m - 900, rng.integers(0, 3, m - 900))])
    recs["block_id"][1000:1006] = recs["block_id"][950]
    owners = np.where(np.arange(m) < 900, 0, 1)
    _place(rng, recs, 2, owners)
    tbl = ds.table(range(3))
    _, _, info1 = ds.model(recs, 3, tbl)
    mx = info1["max_refs"]
    assert mx == 7
    base = node.dict_create(recs, tbl, mode=MODES["copy"])
    for min_refs in (0, 1, 2, 3, mx, mx + 1, 0xFFFFFFFF):
        out, exp = _check(node, plain, recs, 3, tbl, "copy", min_refs, tag=f"min_refs={min_refs}", base=base, rng=rng)
        eo = dc.owner_of(exp["block_id"], 2) if len(exp) else np.zeros(0, np.int64)
        if min_refs == 3:
            assert (eo == 0).sum() >= 290 and (eo == 1).sum() == 1
        if min_refs == mx:
            assert len(exp) == 1 and eo[0] == 1
        if min_refs > mx:
            assert out.entries == 0
        out.release()
    # above every count: 0 entries, 0 blobs, answers nothing, can be extended
    z, info = node.dict_distill_parts(base, mx + 1)
    zi = z.info()
    assert (z.entries, zi["blobs"], zi["record_capacity"]) == (0, 0, 0)
    assert (info["entries_out"], info["blobs_out"], info["below_min"]) == (0, 0, info["distinct"])
    q = _queries(rng, recs)
    got, gtbl = node.dict_export_parts(z)
    assert len(got) == 0 and gtbl is None
    _node_answers("a dict of nothing", node, z, got, q)
    E = ds.rows(rng, 50, 0)
    E["block_id"][:10] = q[:10]
    z1 = node.dict_extend(z, E, ds.table([77]))
    assert (_hits(E, q)["entry"] != nydus_gpu.MISS).sum() == 10
    _node_answers("extend of a dict of nothing", node, z1, E, q)
    _export_equals("extend of a dict of nothing", node, z1, E, ds.table([77]))
    for h in (z1, z, base):
        h.release()
    for e in node.engines:
        e.device_status()


# ---- 5: crafted part tables --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed"])
def test_crafted_part_tables(mode, node_of, plain):
    """node_cases' dict for W = 3: in every part's own table a tag chain on unequal
    digests (with the two repeats it carries), a chain homed two slots before the
    end (it wraps), and the 0xFFFFFFFF / 0xFFFFFFFE tag pairs.  More repeats are
    added behind every other member of their chains, without moving a part's table
    capacity; the ones node_cases shuffles in stand before other members."""
    W = 3
    node = node_of(W)
    nd = nc.get_dict(W, "full")
    dd, dsz, db, di, duoff, nb = nd.rows
    rows = np.zeros(len(dsz), rafs.CHUNK_INFO_DTYPE)
    rows["block_id"], rows["uncompressed_size"], rows["blob_index"] = dd, dsz, db
    rows["index"], rows["uncompressed_offset"] = di, duoff
    rows["compressed_offset"] = np.arange(len(rows), dtype=np.uint64) * 4096 + 17
    rows["compressed_size"], rows["flags"] = 4000, 1
    chains = nd.row_classes["part_tagchain"]
    wraps = nd.row_classes["part_wrap"]
    tagff = nd.row_classes["tagff"]
    # a repeat that stands before another member of its chain
    assert any(min(int(r) for r in g[nc.CHAIN:]) < max(int(r) for r in g[:nc.CHAIN]) for g in chains)
    want = [int(g[3]) for g in chains] + [int(g[0]) for g in wraps] + [int(chains[0][3])] + \
           [int(g[5]) for g in chains] + [int(g[3]) for g in wraps] + [int(g[-1]) for g in tagff]
    room = [(c - 16) // 2 - p for c, p in zip(nd.cap, nd.pm)]  # rows a part takes before its table grows
    again = []
    for r in want:
        o = int(nd.owners[r])
        if room[o]:
            room[o] -= 1
            again.append(r)
    assert len(again) >= 2 * W + 1
    more = rows[again].copy()
    more["blob_index"] = nc.DUP_BLOB
    more["index"] += 7
    recs = np.concatenate([rows, more])
    pm = np.bincount(dc.owner_of(recs["block_id"], W), minlength=W)
    assert [nc.part_cap(int(x)) for x in pm] == nd.cap  # the wrap rows are still homed at cap - 2
    win, refs = ds.refs_of(recs)
    assert refs[int(chains[0][3])] == 3 and refs[int(chains[0][0])] == 2 and refs[int(wraps[1][0])] == 2
    rng = np.random.default_rng(9600)
    q = np.ascontiguousarray(np.stack([x[1] for x in nd.queries] + [recs["block_id"][r] for r in again]))
    base = node.dict_create(recs, mode=MODES[mode])
    assert base.info()["blobs"] == nb
    seen = set()
    for min_refs in (1, 2, 3, 4):
        out, exp = _check(node, plain, recs, nb, None, mode, min_refs, tag=f"crafted {mode} min_refs={min_refs}",
                          base=base, rng=rng, q=q)
        seen.add(len(exp))
        out.release()
    assert len(seen) == 4 and 0 in seen
    base.release()
    for e in node.engines:
        e.device_status()


# ---- 6: handles --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed"])
def test_handles_growth_save_and_placements(mode, node_of, plain, tmp_path):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(9700 + (mode == "routed"))
    R1 = ds.pattern("triples", rng, 3000, nb=3)
    R1["blob_index"][:3] = (0, 1, 2)
    _place(rng, R1, W)
    R2 = ds.rows(rng, 300, rng.integers(0, 2, 300))
    R2["blob_index"][:2] = (0, 1)
    R2["block_id"][:100] = R1["block_id"][5:305:3]  # digests the older handle holds
    R2["block_id"][100:150] = R2["block_id"][150:200]
    b = node.dict_create(R1, mode=MODES[mode])
    # room first: a retire of nothing leaves every part room for half its rows again
    c = node.dict_retire_parts(b, [])
    x1 = node.dict_extend(c, R2)
    assert x1.info()["shares_base_storage"]
    x1_rows = _appended(R1, 3, R2)
    # the older handle distils only its own rows, with R2's rows and slots on its storages
    o_c, e_c = _check(node, plain, R1, 3, None, mode, 1, tag=f"{mode} older handle", base=c, rng=rng)
    o_x, e_x = _check(node, plain, x1_rows, 5, None, mode, 1, tag=f"{mode} newer handle", base=x1, rng=rng)
    assert len(e_x) > len(e_c)
    for min_refs in (2, 3, 4):
        for rows, nb, h in ((R1, 3, c), (x1_rows, 5, x1)):
            o, _ = _check(node, plain, rows, nb, None, mode, min_refs, tag=f"{mode} handles min_refs={min_refs}",
                          base=h, rng=rng, probe=False)
            o.release()
    # after a distill, extends and node folds of up to s_o / 2 rows per part append in place
    i0 = o_c.info()
    s_part = np.bincount(dc.owner_of(e_c["block_id"], W), minlength=W)
    E = ds.rows(rng, 150, 0)
    E["block_id"][:20] = e_c["block_id"][:20]  # the survivors' rows win
    e1 = node.dict_extend(o_c, E)
    assert e1.info()["shares_base_storage"] and e1.info()["record_capacity"] == i0["record_capacity"]
    nbc = i0["blobs"]
    e_rows = _appended(e_c, nbc, E)
    parts = [_tables(rng, 40, rng.random(40) < 0.5) + (None,) for _ in range(W)]
    pl = _places(rng, sum(_k_of(parts)))
    new_rows, B = _node_model(parts, pl)
    grown = np.bincount(dc.owner_of(np.concatenate([E["block_id"], new_rows["block_id"]]), W), minlength=W)
    assert (grown <= s_part // 2).all(), (grown, s_part)
    g1 = _nfold(node, e1, parts, pl)
    assert g1.info()["shares_base_storage"] and g1.info()["record_capacity"] == i0["record_capacity"]
    g_rows = _appended(e_rows, nbc + 1, new_rows)
    _export_equals(f"{mode} distill -> extend", node, e1, e_rows, None)
    _export_equals(f"{mode} distill -> extend -> fold", node, g1, g_rows, None)
    q = _queries(rng, g_rows, [R1["block_id"][::9]])
    _node_answers(f"{mode} distill -> extend -> fold", node, g1, g_rows, q)
    _node_answers(f"{mode} blind to both", node, o_c, e_c, q)
    # ... and a distill of the grown dict drops E's 20 shadows again
    o_g, e_g = _check(node, plain, g_rows, nbc + 1 + B, None, mode, 1, tag=f"{mode} again", base=g1, rng=rng)
    assert len(e_g) == len(g_rows) - 20
    # save, then open: the same rows and blob rows
    t3 = ds.table(range(3))
    bt = node.dict_create(R1, t3, mode=MODES[mode])
    o_t, info_t = node.dict_distill_parts(bt, 2)
    e_t, etbl, einfo = ds.model(R1, 3, t3, 2)
    assert info_t == einfo
    path = str(tmp_path / f"distilled-{mode}.boot")
    info = node.dict_save(o_t, path)
    assert info["entries"] == len(e_t)
    back = node.dict_open(path, MODES[mode])
    _export_equals(f"{mode} save and open", node, back, e_t, etbl)
    # placement rows follow the survivors (the exports above compare them); a base
    # that keeps none gives a result that keeps none: a fold with no placements
    # onto an empty dict, twice, so that every digest is held by two rows
    assert (e_x["compressed_size"] != e_x["uncompressed_size"]).any() and e_x["compressed_offset"].any()
    empty = node.dict_create(R1[:0], mode=MODES[mode])
    f1 = _nfold(node, empty, parts)
    f2 = _nfold(node, f1, parts)
    bare, Bb = _node_model(parts, None)
    bare2 = _appended(bare, Bb, bare)
    _export_equals(f"{mode} no placements base", node, f2, bare2, None)
    o_b, e_b = _check(node, plain, bare2, 2 * Bb, None, mode, 2, tag=f"{mode} no placements", base=f2, rng=rng,
                      probe=False)
    assert len(e_b) == len(bare) and not e_b["compressed_offset"].any()
    assert (e_b["compressed_size"] == e_b["uncompressed_size"]).all()
    for h in (o_b, f2, f1, empty, back, o_t, bt, o_g, g1, e1, o_x, o_c, x1, c, b):
        h.release()
    for e in node.engines:
        e.device_status()


# ---- 7: real layers ------------------------------------------------------------------------
def test_step_and_streaming_pack_against_a_distilled_dict(oracle):
    """A partitioned dict of two real layers' chunks (the digests of real tar chunks,
    so the owners are whatever the digests say and the survivors lie on both sides
    of the owner boundary), every digest of the first layer on two or three rows
    among single ones: Node.process_step over both layers and a streaming Node.pack
    of each against distill_parts(dict, 2) equal the oracle fed the model's rows,
    and, byte for byte, the same calls against a dict created from them."""
    import layers
    import torch
    cs = CS
    rng = np.random.default_rng(9800)
    lay = [layers.edge_tar(chunk=cs), layers.oci_upper_tar_go(2)]
    chs = [oracle.tar_chunks(t, cs) for t in lay]
    digs = [oracle.digest_chunks(t, c, "blake3") for t, c in zip(lay, chs)]
    n0 = len(digs[0])

    def recs(dig, length, blob):
        r = ds.rows(rng, len(dig), blob, cs)
        r["block_id"], r["uncompressed_size"] = dig, length
        return r
    front = recs(digs[0][:n0 // 2], chs[0]["length"][:n0 // 2], 0)
    mid = recs(digs[0], chs[0]["length"], rng.integers(1, 3, n0))
    back = recs(digs[0], chs[0]["length"], 3)
    other = recs(digs[1][::2], chs[1]["length"][::2], rng.integers(0, 4, len(digs[1][::2])))
    rows = np.concatenate([front, ds.rows(rng, 2000, rng.integers(0, 4, 2000), cs), mid, other, back])
    tbl = ds.table(range(4), cs)
    frows, ftbl, finfo = ds.model(rows, 4, tbl, 2)
    own = dc.owner_of(frows["block_id"], 2)
    assert 0 < (own == 0).sum() < len(frows)  # survivors on both sides of the owner boundary

    def expect(r, i):
        dec, _ = oracle.dedup(digs[i], chs[i]["length"], r["block_id"], r["uncompressed_size"], r["blob_index"],
                              r["index"], dict_uoff=r["uncompressed_offset"])
        return dec

    node = nydus_gpu.Node([0, 0], chunk_size=cs)
    try:
        d = node.dict_create(rows, tbl, mode=MODES["copy"])
        ret, info = node.dict_distill_parts(d, 2)
        assert info == finfo
        one = node.dict_create(frows, np.frombuffer(ftbl, np.uint8), mode=MODES["copy"])
        assert node.dict_export_parts(ret)[0].tobytes() == frows.tobytes()
        keep, parts = [], []
        for t, c in zip(lay, chs):
            buf = torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda()
            dch = torch.from_numpy(np.ascontiguousarray(c).view(np.uint8).copy()).cuda()
            keep.append((buf, dch))
            parts.append({"d_data": buf.data_ptr(), "len": buf.numel(), "d_chunks": dch.data_ptr(), "n": len(c)})

        def step(h):
            outs = [torch.zeros(len(c) * 64, dtype=torch.uint8, device="cuda") for c in chs]
            torch.cuda.synchronize()
            node.process_step(h, [dict(p, d_out=o.data_ptr()) for p, o in zip(parts, outs)])
            torch.cuda.synchronize()
            return [o.cpu().numpy().view(nydus_gpu.RESULT_DTYPE) for o in outs]

        def packs(h):
            res = []
            for t in lay:
                w = node.pack(dict=h)
                w.write(t)
                res.append(w.close())
            return res

        got_step, one_step, base_step = step(ret), step(one), step(d)
        got_pack, one_pack = packs(ret), packs(one)
        changed = False
        for i in range(2):
            dec_f, dec_0 = expect(frows, i), expect(rows, i)
            changed = changed or dec_f.tobytes() != dec_0.tobytes()
            for tag, got, dec in (("step", got_step[i], dec_f), ("step base", base_step[i], dec_0),
                                  ("pack", got_pack[i][1], dec_f)):
                assert np.array_equal(got["digest"], digs[i]), (tag, i)
                for f in ("kind", "index", "blob_index"):
                    assert np.array_equal(got[f], dec[f]), (tag, i, f)
            assert got_step[i].tobytes() == one_step[i].tobytes(), i
            assert got_pack[i][0].tobytes() == one_pack[i][0].tobytes() == np.ascontiguousarray(chs[i]).tobytes()
            assert got_pack[i][1].tobytes() == one_pack[i][1].tobytes(), i
            assert got_pack[i][2] == one_pack[i][2], i
        assert changed and (expect(frows, 0)["kind"] == nydus_gpu.DICT).sum() > 0
        for h in (one, ret, d):
            h.release()
    finally:
        node.close()


# ---- 8: refusals -----------------------------------------------------------------------------
def test_refusals_and_the_old_call_next_to_the_new_one(node_of, plain):
    W = 3
    node = node_of(W)
    L = nydus_gpu.lib()
    rng = np.random.default_rng(9900)
    recs = ds.pattern("triples", rng, 600, nb=4)
    recs["blob_index"][:4] = np.arange(4)
    _place(rng, recs, W)
    tbl = ds.table(range(4))
    q = _queries(rng, recs)

    def raw(fn, nd, d, min_refs=1, flags=0, with_out=True):
        h, info = ctypes.c_void_p(0xDEAD), nydus_gpu.NgpuDictDistillInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
        rc = fn(nd._h, d._h, min_refs, flags, ctypes.byref(h) if with_out else None, ctypes.byref(info))
        return rc, (h.value if with_out else None), bytes(info) == bytes(312)

    new, old = L.ngpu_node_dict_distill_parts, L.ngpu_node_dict_distill
    p = node.dict_create(recs, tbl, mode=MODES["copy"])
    _node_answers("base before", node, p, recs, q)
    # the old call keeps its answer for a partitioned dict
    for with_out in (True, False):
        assert raw(old, node, p, with_out=with_out) == (nydus_gpu.EUNSUPP, None, True)
    with pytest.raises(nydus_gpu.NgpuError) as x:
        node.dict_distill(p, 1)
    assert x.value.code == nydus_gpu.EUNSUPP
    # flags
    for flags in (0x4, KEEP | MERGE, 0x80000000):
        for with_out in (True, False):
            assert raw(new, node, p, 1, flags, with_out) == (nydus_gpu.EINVAL, None, True)
    # a plain dict
    pd = plain.dict_create(recs, tbl)
    for with_out in (True, False):
        assert raw(new, node, pd, with_out=with_out) == (nydus_gpu.EINVAL, None, True)
    pd.release()
    # a dict of another node
    other = nydus_gpu.Node([0, 0], chunk_size=CS)
    try:
        for with_out in (True, False):
            assert raw(new, other, p, with_out=with_out) == (nydus_gpu.EINVAL, None, True)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            other.dict_distill_parts(p)
        assert x.value.code == nydus_gpu.EINVAL
    finally:
        other.close()
    # MERGE_BLOB_IDS without a blob table
    bare = node.dict_create(recs, mode=MODES["copy"])
    for with_out in (True, False):
        assert raw(new, node, bare, 1, MERGE, with_out) == (nydus_gpu.EINVAL, None, True)
    bare.release()
    # ... and the base answers as before all of the above, and distils
    _node_answers("base after the refusals", node, p, recs, q)
    out, _ = _check(node, plain, recs, 4, tbl, "copy", 2, tag="after the refusals", base=p, rng=rng, q=q)
    out.release()
    p.release()
    # a replicated dict through the new call equals the old call
    r = node.dict_create(recs, tbl, mode=MODES["replicate"])
    for min_refs, flags in ((1, 0), (3, 0), (2, KEEP), (1, MERGE)):
        (a, ia), (b, ib) = node.dict_distill_parts(r, min_refs, **_kw(flags)), node.dict_distill(r, min_refs, **_kw(flags))
        exp, etbl, einfo = ds.model(recs, 4, tbl, min_refs, flags)
        assert ia == ib == einfo and a.info() == b.info()
        ea, eb = node.dict_export_parts(a), node.dict_export(b)
        assert ea[0].tobytes() == eb[0].tobytes() == exp.tobytes() and ea[1] == eb[1] == etbl
        assert node.dict_distill_parts(r, min_refs, count_only=True, **_kw(flags)) == \
            node.dict_distill(r, min_refs, count_only=True, **_kw(flags)) == (None, einfo)
        a.release()
        b.release()
    r.release()
    for e in node.engines:
        e.device_status()
