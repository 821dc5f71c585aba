"""Retire and export of node dicts across their parts (ngpu_node_dict_retire_parts /
ngpu_node_dict_export, csrc/node.hip + csrc/node_retire.hip) on the GPU, on nodes
that list device 0 W times.

The expectation everywhere is the header's definition: the base's rows in global
table order without those of the listed blobs, kept blobs re-ranked --
test_gpu_dict_retire._filtered.  A result is compared three ways: byte for byte
through Node.dict_export_parts; through the product path (engines[i].set_dict +
ngpu_dedup_device on every engine of the node: every result field and every stats
field) against a plain Engine.dict_create of the filtered rows; and against a
Node.dict_create of the filtered rows in the same mode.

  1  export alone: create, extend, fold (a partitioned fold compared byte for byte),
     with and without placement rows, create(export(d)) answers as d
  2  compaction edges: W in 2, 3, 5, 8, both exchanges; global m where a keep word
     and a scan tile end; owners crafted so that a part owns 0, 1, 63, ... 257 rows,
     nothing, or everything; every keep pattern; 63 / 64 / 65 blobs with a table
  3  first entry wins after the winner leaves; node_cases' crafted part tables with
     a chain member retired at each position
  4  handles: base untouched, older handles, retire -> extend -> fold share, chains
  5  real layers: Node.process_step and a streaming Node.pack against the result
  6  refusals, and the old calls' answers next to the new ones
"""
import ctypes

import numpy as np
import pytest

import dedup_cases as dc
import node_cases as nc
import nydus_gpu
from nydus_gpu import rafs
from test_gpu_dict_fold import DICT, _appended, _dev, _places, _tables
from test_gpu_dict_retire import (_caps, _filtered, _first_rows, _keep_patterns, _rows, _same_rows, _table,
                                  _table_rows)
from test_gpu_node_fold import MODES, _agree, _ask, _k_of, _nfold, _node_model

pytestmark = pytest.mark.gpu

CS = 0x10000
T = 256 * 64  # ids per scan tile of the retire: kRetireScanTile keep words of 64
GLOBAL_M = [0, 1, 63, 64, 65, 4097, T + 1, 2 * T + 1]
PART_M = [0, 1, 63, 64, 65, 255, 256, 257]


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


def _set_owners(rng, rows, owners, W):
    """Digest prefixes (the first 16 bits) drawn from each row's owner's range."""
    o = np.asarray(owners, np.int64)
    lo, hi = -(-o * 65536 // W), -(-(o + 1) * 65536 // W) - 1
    p = rng.integers(lo, hi + 1) if len(o) else np.zeros(0, np.int64)
    rows["block_id"][:, 0] = p >> 8
    rows["block_id"][:, 1] = p & 0xFF
    assert (dc.owner_of(rows["block_id"], W) == o).all()
    return rows


def _owners(rng, m, W, layout, shift=0):
    if layout == "one_owner":       # part W - 1 owns every row
        return np.full(m, W - 1, np.int64)
    if layout == "one_empty":       # part W // 2 owns nothing
        o = rng.integers(0, W - 1, m)
        o[o >= W // 2] += 1
        return o
    if layout == "spread":
        return rng.integers(0, W, m)
    # "sizes": part i owns PART_M[(shift + i) % 8] rows while they fit, the last part
    # the rest; the parts' rows interleave in table order
    counts, left = [], m
    for i in range(W - 1):
        c = min(PART_M[(shift + i) % len(PART_M)], left)
        counts.append(c)
        left -= c
    counts.append(left)
    return rng.permutation(np.repeat(np.arange(W), counts))


def _sample_query(rng, kept, gone=None, cap=3000):
    """Up to `cap` surviving digests, some of the retired ones and fresh misses, at
    the rows' sizes, shuffled."""
    def pick(r, k):
        return r if len(r) <= k else r[np.sort(rng.choice(len(r), k, replace=False))]
    parts = [pick(kept, cap)] + ([] if gone is None else [pick(gone, cap // 4)])
    q = np.concatenate([p["block_id"] for p in parts] + [rng.integers(0, 256, (64, 32), dtype=np.uint8)])
    us = np.concatenate([p["uncompressed_size"] for p in parts] + [np.full(64, CS, np.uint32)])
    lens = np.where(us == 0, CS, us).astype(np.uint32)
    order = rng.permutation(len(q))
    return np.ascontiguousarray(q[order]), lens[order]


def _export_equals(tag, node, d, rows, tbl):
    got, gtbl = node.dict_export_parts(d)
    _same_rows(got, rows, tag)
    if tbl is not None and not isinstance(tbl, bytes):
        tbl = np.ascontiguousarray(tbl).tobytes()
    assert gtbl == tbl, tag
    return got, gtbl


def _answers_as(tag, node, plain, handles, rows, mode, q, lens):
    """Every handle, on every engine of the node, answers the queries as a plain
    Engine dict of `rows` and as a node dict created from them in the same mode."""
    pd = plain.dict_create(rows)
    one = node.dict_create(rows, mode=MODES[mode])
    try:
        ref = _ask(plain, pd, q, lens)
        for name, d in list(handles.items()) + [("create", one)]:
            assert d.entries == len(rows), (tag, name)
            for i, e in enumerate(node.engines):
                _agree(f"{tag} {name} engine {i}", _ask(e, d, q, lens), ref)
        return ref
    finally:
        plain.set_dict(None)
        for e in node.engines:
            e.set_dict(None)
        one.release()
        pd.release()


def _three_ways(tag, node, plain, out, frows, ftbl, mode, q, lens):
    _export_equals(tag, node, out, frows, ftbl)
    return _answers_as(tag, node, plain, {"retired": out}, frows, mode, q, lens)


# ---- 1: export alone ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed", "replicate"])
def test_export_alone_create_extend_fold(mode, node_of, plain):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(11)
    tbl = _table(3, CS)
    for m in (0, 1, 65, 3001):
        rows = _rows(rng, m, rng.integers(0, 3, m), CS)
        if m:
            rows["blob_index"][-1] = 2
        for with_tbl in (True, False):
            tag = f"{mode} m={m} table={with_tbl}"
            d = node.dict_create(rows, tbl if with_tbl else None, mode=MODES[mode])
            got, gtbl = _export_equals(tag, node, d, rows, tbl if with_tbl else None)
            if mode == "replicate":  # the old call's answer, byte for byte
                old, otbl = node.dict_export(d)
                assert old.tobytes() == got.tobytes() and otbl == gtbl
            # create(export(d)) answers as d
            one = node.dict_create(got, None if gtbl is None else np.frombuffer(gtbl, np.uint8), mode=MODES[mode])
            assert one.info()["entries"] == d.info()["entries"] and one.info()["blobs"] == d.info()["blobs"]
            assert node.dict_export_parts(one)[0].tobytes() == got.tobytes()
            if m:
                q, lens = _sample_query(rng, rows)
                _answers_as(tag, node, plain, {"dict": d, "create(export)": one}, rows, mode, q, lens)
            one.release()
            d.release()
    # after an extend and after a fold, with placement rows
    rows = _rows(rng, 2000, rng.integers(0, 2, 2000), CS)
    rows["blob_index"][0] = 1
    more = _rows(rng, 700, 0, CS)
    d = node.dict_create(rows, mode=MODES[mode])
    x = node.dict_extend(d, more)
    x_rows = _appended(rows, 2, more)
    _export_equals(f"{mode} extend", node, x, x_rows, None)
    parts = [_tables(rng, n, rng.random(n) < 0.6) + (None,) for n in (257, 64, 1025)]
    pl = _places(rng, sum(_k_of(parts)))
    frows, B = _node_model(parts, pl)
    f = _nfold(node, x, parts, pl)
    f_rows = _appended(x_rows, 3, frows)
    assert f.info()["blobs"] == 3 + B
    _export_equals(f"{mode} fold", node, f, f_rows, None)
    _export_equals(f"{mode} fold base", node, x, x_rows, None)
    q, lens = _sample_query(rng, f_rows)
    _answers_as(f"{mode} fold", node, plain, {"fold": f}, f_rows, mode, q, lens)
    # without placement rows: a fold onto an empty dict with no placements given
    e = node.dict_create(rows[:0], mode=MODES[mode])
    g = _nfold(node, e, parts)
    bare, _ = _node_model(parts, None)
    assert (bare["compressed_size"] == bare["uncompressed_size"]).all() and not bare["compressed_offset"].any()
    _export_equals(f"{mode} fold without placements", node, g, bare, None)
    for h in (g, e, f, x, d):
        h.release()
    for eng in node.engines:
        eng.device_status()


# ---- 2: compaction edges -----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed"])
@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_compaction_edges(W, mode, node_of, plain):
    """Kept rows are blob 0, retired rows blob 1 of a 2-blob table.  Every result is
    compared byte for byte through the export; the random pattern, a part whose
    rows all leave, and the one-owner layout also through the product path."""
    node = node_of(W)
    rng = np.random.default_rng(2000 + 10 * W + (mode == "routed"))
    tbl = _table(2, CS)
    seen_part_m, asked = set(), 0
    for mi, m in enumerate(GLOBAL_M):
        plans = [("sizes", mi, None), ("one_owner", 0, ("random", "none", "all")),
                 ("one_empty", 0, ("random", "runs"))]
        if m == GLOBAL_M[-1]:  # every part size of PART_M on this W
            plans += [("sizes", s, ("random",)) for s in range(len(PART_M)) if s != mi]
        for layout, shift, only in plans:
            owners = _owners(rng, m, W, layout, shift)
            rows = _set_owners(rng, _rows(rng, m, 0, CS), owners, W)
            part_m = np.bincount(owners, minlength=W)
            seen_part_m.update(int(x) for x in part_m)
            if layout == "one_owner" and m:
                assert sorted(part_m)[:-1] == [0] * (W - 1)
            if layout == "one_empty" and m > 64:
                assert part_m[W // 2] == 0 and (np.delete(part_m, W // 2) > 0).all()
            patterns = list(_keep_patterns(m, rng))
            big = int(np.argmax(part_m))
            if m > 1 and layout != "one_owner":  # a part whose rows all leave while others stay
                patterns.append(("part leaves", owners != big))
            for name, keep in patterns:
                if only is not None and name not in only:
                    continue
                tag = f"W={W} {mode} m={m} {layout}/{shift} {name}"
                rows["blob_index"] = np.where(keep, 0, 1)
                exp, kept = _filtered(rows, [1], 2)
                assert len(exp) == int(keep.sum())
                base = node.dict_create(rows, tbl, mode=MODES[mode])
                out = node.dict_retire_parts(base, [1])
                info = out.info()
                assert (info["entries"], info["blobs"]) == (len(exp), 1), (tag, info)
                s0 = int((keep & (owners == 0)).sum())
                assert (info["record_capacity"], info["table_capacity"]) == _caps(s0), (tag, info)
                assert not info["shares_base_storage"], tag
                _export_equals(tag, node, out, exp, _table_rows(tbl, kept))
                if name in ("random", "part leaves") and layout != "one_empty" and len(exp):
                    q, lens = _sample_query(rng, exp, rows[~keep])
                    _answers_as(tag, node, plain, {"retired": out}, exp, mode, q, lens)
                    asked += 1
                if name == "random":  # the base is as it was
                    _export_equals(tag + " base", node, base, rows, tbl)
                out.release()
                base.release()
    assert seen_part_m >= set(PART_M), sorted(seen_part_m)
    assert asked >= 6
    for e in node.engines:
        e.device_status()


@pytest.mark.parametrize("nb", [63, 64, 65])
def test_blob_counts_with_a_table(nb, node_of, plain):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(nb)
    m = 1000
    rows = _rows(rng, m, rng.integers(0, nb, m), CS)
    rows["blob_index"][:nb] = np.arange(nb)  # every blob has a row
    tbl = _table(nb, CS)
    base = node.dict_create(rows, tbl, mode=MODES["copy"])
    for gone in ([0], [nb - 1], list(range(0, nb, 2)), list(range(1, nb, 2)), [nb - 1, 0, nb - 1]):
        exp, kept = _filtered(rows, gone, nb)
        out = node.dict_retire_parts(base, gone)
        assert out.info()["blobs"] == len(kept)
        got, gtbl = _export_equals(f"nb={nb} gone={gone[:3]}", node, out, exp, _table_rows(tbl, kept))
        by_id = node.dict_retire_parts(base, [f"{b:064x}" for b in gone])  # ids name the same blobs
        assert node.dict_export_parts(by_id)[0].tobytes() == got.tobytes()
        by_id.release()
        out.release()
    exp, kept = _filtered(rows, [1, nb - 2], nb)
    out = node.dict_retire_parts(base, [nb - 2, 1])
    q, lens = _sample_query(rng, exp, rows[np.isin(rows["blob_index"], [1, nb - 2])])
    _three_ways(f"nb={nb}", node, plain, out, exp, _table_rows(tbl, kept), "copy", q, lens)
    with pytest.raises(ValueError):
        node.dict_retire_parts(base, ["ee" * 32])
    out.release()
    base.release()


# ---- 3: first entry wins after the winner leaves -----------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed"])
def test_first_entry_wins_after_the_winner_leaves(mode, node_of, plain):
    """40 digests on three rows each, in blobs 0, 1 and 2 (one owner by construction:
    the owner is the digest's prefix), among filler rows of blob 3.  With blob 0
    retired the blob-1 row answers, with blobs 0 and 1 retired the blob-2 row."""
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(33)
    fill = _rows(rng, 600, 3, CS)
    trip = [_rows(rng, 40, b, CS) for b in range(3)]
    for t in trip[1:]:
        t["block_id"] = trip[0]["block_id"]
    # table order: front copies, filler, middle copies, filler, back copies
    rows = np.concatenate([trip[0], fill[:300], trip[1], fill[300:], trip[2]])
    base = node.dict_create(rows, mode=MODES[mode])
    q = np.concatenate([trip[0]["block_id"], fill["block_id"][::7], rng.integers(0, 256, (16, 32), dtype=np.uint8)])
    lens = np.full(len(q), CS, np.uint32)
    answers = []
    for gone, winner in (([], 0), ([0], 1), ([0, 1], 2), ([1], 0), ([0, 1, 2], None)):
        frows, kept = _filtered(rows, gone, 4)
        out = node.dict_retire_parts(base, gone)
        ref, _ = _three_ways(f"{mode} gone={gone}", node, plain, out, frows, None, mode, q, lens)
        first = _first_rows(frows["block_id"])
        for i in range(40):  # the triple's digests: the next survivor's row answers
            j = first.get(bytes(q[i]))
            if winner is None:
                assert j is None and ref["kind"][i] != DICT
            else:
                assert ref["kind"][i] == DICT and ref["index"][i] == frows["index"][j] == trip[winner]["index"][i]
        answers.append(ref.tobytes())
        out.release()
    assert len(set(answers)) == 5  # every retire set changes the answers (entry ids and blob ranks too)
    base.release()


@pytest.mark.parametrize("mode", ["copy", "routed"])
def test_crafted_part_tables_with_every_chain_position_retired(mode, node_of, plain):
    """node_cases' dict for W = 3 (per part a tag chain with repeats and a wrapping
    chain, the 0xFFFFFFFF / 0xFFFFFFFE tag pairs): every member of those groups sits
    in a blob of its own and is retired in turn, then each whole group."""
    W = 3
    node = node_of(W)
    nd = nc.get_dict(W, "full")
    dd, ds, db, di, duoff, nb0 = nd.rows
    rows = np.zeros(len(ds), rafs.CHUNK_INFO_DTYPE)
    rows["block_id"], rows["uncompressed_size"], rows["blob_index"] = dd, ds, db
    rows["index"], rows["uncompressed_offset"] = di, duoff
    rows["compressed_offset"] = np.arange(len(rows), dtype=np.uint64) * 4096 + 17
    rows["compressed_size"], rows["flags"] = 4000, 1
    groups = [g for c in ("part_tagchain", "part_wrap", "tagff") for g in nd.row_classes[c]]
    special = [int(r) for g in groups for r in g]
    assert len(special) == len(set(special)) >= W * (nc.CHAIN + 2 + nc.WRAP)
    rows["blob_index"][special] = nb0 + np.arange(len(special))
    nb = nb0 + len(special)
    blob_of = {r: nb0 + k for k, r in enumerate(special)}
    sets = [[blob_of[r]] for r in special] + [[blob_of[int(r)] for r in g] for g in groups]
    rng = np.random.default_rng(35)
    qd = np.stack([x[1] for x in nd.queries] + [rows["block_id"][r] for r in special])
    ql = np.array([x[2] for x in nd.queries] + [CS] * len(special), np.uint32)
    base = node.dict_create(rows, mode=MODES[mode])
    before = [_ask(e, base, qd, ql) for e in node.engines]
    seen = set()
    for gone in sets:
        frows, kept = _filtered(rows, gone, nb)
        out = node.dict_retire_parts(base, gone)
        assert out.info()["blobs"] == len(kept)
        ref, _ = _three_ways(f"{mode} gone={gone}", node, plain, out, frows, None, mode, qd, ql)
        seen.add(ref.tobytes())
        out.release()
    assert len(seen) > len(groups)  # the retired members did answer before
    for e, b in zip(node.engines, before):
        _agree("base after the retires", _ask(e, base, qd, ql), b)
        e.set_dict(None)
    base.release()


# ---- 4: handles --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed"])
def test_handles_base_untouched_older_handles_and_growth_after_retire(mode, node_of, plain):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(44)
    R1 = _rows(rng, 1000, rng.integers(0, 3, 1000), CS)
    R1["blob_index"][:3] = (0, 1, 2)
    R2 = _rows(rng, 400, rng.integers(0, 2, 400), CS)
    R2["blob_index"][:2] = (0, 1)
    R3 = _rows(rng, 300, 0, CS)
    R3["block_id"][:50] = R1["block_id"][100:150]  # digests x1 already holds
    b = node.dict_create(R1, mode=MODES[mode])
    x1 = node.dict_extend(b, R2)  # every part forks
    x1_rows = _appended(R1, 3, R2)
    q, lens = _sample_query(rng, np.concatenate([x1_rows, R3]))
    # the base answers exactly as before the call
    info0 = x1.info()
    before = [_ask(e, x1, q, lens) for e in node.engines]
    r1 = node.dict_retire_parts(x1, [1, 4])
    assert x1.info() == info0
    for e, a in zip(node.engines, before):
        _agree("base after", _ask(e, x1, q, lens), a)
    _export_equals("base after", node, x1, x1_rows, None)
    f1, _ = _filtered(x1_rows, [1, 4], 5)
    _three_ways(f"{mode} r1", node, plain, r1, f1, None, mode, q, lens)
    # info(): part 0 sits on a storage with a fork's room for its own survivors
    s0 = int((dc.owner_of(f1["block_id"], W) == 0).sum())
    i1 = r1.info()
    assert (i1["entries"], i1["blobs"]) == (len(f1), 3)
    assert (i1["record_capacity"], i1["table_capacity"], i1["shares_base_storage"]) == _caps(s0) + (False,)
    # an older handle whose parts were extended in place: the appended rows are not seen
    x2 = node.dict_extend(x1, R3)
    assert x2.info()["shares_base_storage"]
    r1b = node.dict_retire_parts(x1, [1, 4])
    _export_equals("older handle", node, r1b, f1, None)
    x2_rows = _appended(x1_rows, 5, R3)
    r2 = node.dict_retire_parts(x2, [0])
    f2, _ = _filtered(x2_rows, [0], 6)
    _three_ways(f"{mode} r2", node, plain, r2, f2, None, mode, q, lens)
    # n == 0: a compacting copy on storages of its own
    c = node.dict_retire_parts(x1, [])
    ic = c.info()
    m0 = int((dc.owner_of(x1_rows["block_id"], W) == 0).sum())
    assert not ic["shares_base_storage"] and ic["record_capacity"] == _caps(m0)[0] and ic["blobs"] == 5
    _export_equals("n == 0", node, c, x1_rows, None)
    # retire -> extend -> fold append in place and equal the model
    E = _rows(rng, len(f1) // 4, 0, CS)
    E["block_id"][:20] = f1["block_id"][:20]  # the survivors' rows win
    e1 = node.dict_extend(r1, E)
    assert e1.info()["shares_base_storage"] and e1.info()["record_capacity"] == i1["record_capacity"]
    e_rows = _appended(f1, 3, E)
    parts = [_tables(rng, 40, rng.random(40) < 0.5) + (None,) for _ in range(W)]
    pl = _places(rng, sum(_k_of(parts)))
    new_rows, B = _node_model(parts, pl)
    g1 = _nfold(node, e1, parts, pl)
    assert g1.info()["shares_base_storage"] and g1.info()["record_capacity"] == i1["record_capacity"]
    g_rows = _appended(e_rows, 4, new_rows)
    q2, lens2 = _sample_query(rng, g_rows, x1_rows)
    _three_ways(f"{mode} retire -> extend", node, plain, e1, e_rows, None, mode, q2, lens2)
    _three_ways(f"{mode} retire -> extend -> fold", node, plain, g1, g_rows, None, mode, q2, lens2)
    _export_equals("r1 is blind to both", node, r1, f1, None)
    # a chain: retire, extend, retire again
    c1 = node.dict_retire_parts(e1, [3])  # E's blob leaves again
    _export_equals("chain 1", node, c1, f1, None)
    c2 = node.dict_extend(c1, R3[:100])
    c2_rows = _appended(f1, 3, R3[:100])
    c3 = node.dict_retire_parts(c2, [0, 2])
    f4, _ = _filtered(c2_rows, [0, 2], 4)
    _three_ways(f"{mode} chain", node, plain, c3, f4, None, mode, q2, lens2)
    # retire all, then extend
    z = node.dict_retire_parts(x1, range(5))
    assert (z.entries, z.info()["blobs"], z.info()["record_capacity"]) == (0, 0, 0)
    got, gtbl = node.dict_export_parts(z)
    assert len(got) == 0 and gtbl is None
    for e in node.engines:
        assert not (_ask(e, z, q, lens)[0]["kind"] == DICT).any()
        e.set_dict(None)
    z1 = node.dict_extend(z, R3)
    _three_ways(f"{mode} extend of an emptied dict", node, plain, z1, R3, None, mode, q, lens)
    for h in (z1, z, c3, c2, c1, g1, e1, c, r2, r1b, x2, r1, x1, b):
        h.release()
    for e in node.engines:
        e.device_status()


# ---- 5: real layers ------------------------------------------------------------------------
def test_step_and_streaming_pack_against_a_retired_dict(oracle):
    """A partitioned dict of two real layers' chunks, every digest of the first
    layer three times over (blob 0 in front, blobs 1 and 2, blob 3 behind);
    Node.process_step over both layers and a streaming Node.pack of each against
    retire_parts(dict, [0, 2]) equal the oracle fed the filtered rows, and, byte for
    byte, the same calls against a dict created from them."""
    import layers
    import torch
    cs = CS
    rng = np.random.default_rng(55)
    lay = [layers.edge_tar(chunk=cs), layers.oci_upper_tar_go(2)]
    chs = [oracle.tar_chunks(t, cs) for t in lay]
    digs = [oracle.digest_chunks(t, c, "blake3") for t, c in zip(lay, chs)]
    n0 = len(digs[0])

    def recs(dig, length, blob):
        r = _rows(rng, len(dig), blob, cs)
        r["block_id"], r["uncompressed_size"] = dig, length
        return r
    front = recs(digs[0][:n0 // 2], chs[0]["length"][:n0 // 2], 0)
    mid = recs(digs[0], chs[0]["length"], rng.integers(1, 3, n0))
    back = recs(digs[0], chs[0]["length"], 3)
    other = recs(digs[1][::2], chs[1]["length"][::2], rng.integers(0, 4, len(digs[1][::2])))
    rows = np.concatenate([front, _rows(rng, 2000, rng.integers(0, 4, 2000), cs), mid, other, back])
    tbl = _table(4, cs)
    gone = [0, 2]
    frows, kept = _filtered(rows, gone, 4)

    def expect(r, i):
        dec, _ = oracle.dedup(digs[i], chs[i]["length"], r["block_id"], r["uncompressed_size"], r["blob_index"],
                              r["index"], dict_uoff=r["uncompressed_offset"])
        return dec

    node = nydus_gpu.Node([0, 0], chunk_size=cs)
    try:
        d = node.dict_create(rows, tbl, mode=MODES["copy"])
        ret = node.dict_retire_parts(d, gone)
        one = node.dict_create(frows, np.frombuffer(_table_rows(tbl, kept), np.uint8), mode=MODES["copy"])
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
        assert changed and (expect(frows, 0)["kind"] == DICT).sum() > 0  # the retired blobs did answer
        for h in (one, ret, d):
            h.release()
    finally:
        node.close()


# ---- 6: refusals -----------------------------------------------------------------------------
def test_refusals_and_the_old_calls_next_to_the_new_ones(node_of, plain):
    W = 3
    node = node_of(W)
    L = nydus_gpu.lib()
    rng = np.random.default_rng(66)
    rows = _rows(rng, 500, rng.integers(0, 4, 500), CS)
    rows["blob_index"][:4] = np.arange(4)
    tbl = _table(4, CS)
    gone = [1, 3]
    idx = np.asarray(gone, np.uint32)
    frows, kept = _filtered(rows, gone, 4)
    q, lens = _sample_query(rng, rows)

    def raw_retire(nd, d, ix):
        h = ctypes.c_void_p(0xDEAD)
        rc = L.ngpu_node_dict_retire_parts(nd._h, d._h, ix.ctypes.data, len(ix), 0, ctypes.byref(h))
        return rc, h.value

    p = node.dict_create(rows, tbl, mode=MODES["copy"])
    before = [_ask(e, p, q, lens) for e in node.engines]
    # a blob index >= blobs(base)
    for bad in ([4], [0, 4], [1, 0xFFFFFFFF], [1 << 20]):
        assert raw_retire(node, p, np.asarray(bad, np.uint32)) == (nydus_gpu.EINVAL, None)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            node.dict_retire_parts(p, bad)
        assert x.value.code == nydus_gpu.EINVAL and "blob" in str(x.value)
    # a plain dict
    pd = plain.dict_create(rows, tbl)
    assert raw_retire(node, pd, idx) == (nydus_gpu.EINVAL, None)
    m, nb = ctypes.c_uint64(7), ctypes.c_uint32(7)
    assert L.ngpu_node_dict_export(node._h, pd._h, None, 0, ctypes.byref(m), None, 0, ctypes.byref(nb), 0) == \
        nydus_gpu.EINVAL
    assert pd.retire(gone).export()[0].tobytes() == frows.tobytes()  # still usable
    pd.release()
    # a dict of another node
    other = nydus_gpu.Node([0, 0], chunk_size=CS)
    try:
        assert raw_retire(other, p, idx) == (nydus_gpu.EINVAL, None)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            other.dict_export_parts(p)
        assert x.value.code == nydus_gpu.EINVAL
    finally:
        other.close()
    # export: a count, a buffer too small (nothing written), a table buffer too small
    ex = L.ngpu_node_dict_export
    assert ex(node._h, p._h, None, 0, ctypes.byref(m), None, 0, ctypes.byref(nb), 0) == 0
    assert (m.value, nb.value) == (500, 4)
    buf, tb = np.full(80 * 500, 0xA5, np.uint8), np.full(256 * 4, 0xA5, np.uint8)
    for cap, bcap in ((499, 4), (500, 3)):
        m.value = nb.value = 7
        rc = ex(node._h, p._h, buf.ctypes.data, cap, ctypes.byref(m), tb.ctypes.data, bcap, ctypes.byref(nb), 0)
        assert rc == nydus_gpu.EINVAL and (m.value, nb.value) == (500, 4)
        assert (buf == 0xA5).all() and (tb == 0xA5).all()
    assert ex(node._h, p._h, buf.ctypes.data, 500, ctypes.byref(m), tb.ctypes.data, 4, ctypes.byref(nb), 1) == \
        nydus_gpu.EINVAL and (buf == 0xA5).all()  # flags
    assert ex(node._h, p._h, buf.ctypes.data, 500, ctypes.byref(m), tb.ctypes.data, 4, ctypes.byref(nb), 0) == 0
    assert buf.tobytes() == rows.tobytes() and tb.tobytes() == np.ascontiguousarray(tbl).tobytes()
    # the old calls keep their answers for a partitioned dict
    h = ctypes.c_void_p(0xDEAD)
    assert L.ngpu_node_dict_retire(node._h, p._h, idx.ctypes.data, len(idx), 0, ctypes.byref(h)) == nydus_gpu.EUNSUPP
    assert h.value is None
    with pytest.raises(nydus_gpu.NgpuError) as x:
        node.dict_export(p)
    assert x.value.code == nydus_gpu.EUNSUPP
    # ... and the base is as usable as before all of the above
    for e, a in zip(node.engines, before):
        _agree("base after the refusals", _ask(e, p, q, lens), a)
        e.set_dict(None)
    out = node.dict_retire_parts(p, gone)
    _three_ways("after the refusals", node, plain, out, frows, _table_rows(tbl, kept), "copy", q, lens)
    out.release()
    p.release()
    # a replicated dict through the new calls equals the old calls byte for byte
    r = node.dict_create(rows, tbl, mode=MODES["replicate"])
    new, old = node.dict_retire_parts(r, gone), node.dict_retire(r, gone)
    assert new.info() == old.info()
    a, b = node.dict_export_parts(new), node.dict_export(old)
    assert a[0].tobytes() == b[0].tobytes() == frows.tobytes() and a[1] == b[1] == _table_rows(tbl, kept)
    a, b = node.dict_export_parts(r), node.dict_export(r)
    assert a[0].tobytes() == b[0].tobytes() == rows.tobytes() and a[1] == b[1]
    for h in (new, old, r):
        h.release()
    for e in node.engines:
        e.device_status()
