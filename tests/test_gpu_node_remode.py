"""Node dict remode (ngpu_node_dict_remode / ngpu_node_dict_info_get, csrc/node.hip +
csrc/node_remode.hip) on the GPU, on nodes that list device 0 W times.

The model is the header's: Node.dict_create(export(base), blobs, mode).  Every case
holds the result to all of these:
  (a) Node.dict_export_parts(out) equals Node.dict_export_parts(base) byte for byte,
      records and blob table;
  (b) the product path (engines[i].set_dict + ngpu_dedup_device, every result field
      and every stats field) on every engine of the node equals the same call
      against the dict_create model in the target mode and against a plain Engine's
      dict_create of the same rows;
  (c) Node.dict_info(out): the mode asked for, parts == W, entries == m,
      part_entries as dedup_cases.owner_of counts them (replicated: m), zeros past W;
      and every part on a storage with ngpu_dict_retire's room;
  (d) the export of base, and its answers, are unchanged afterwards.

  1  sizes where a wave, a keep word, a 256-row tile and a scan tile end, both
     directions, W in 2, 3, 5, 8, both exchanges, the join at every window width
  2  owners: one part owns every row, one owns none, owners alternate, runs of 64 / 65
  3  first entry wins on node_cases' crafted part tables, after a split and a join
  4  round trips, and the same-mode calls
  5  handles: older handles, growth in place after a remode, retire / distill / save of
     the result, placement rows and blob tables kept iff base had them, 63 / 64 / 65 blobs
  6  real layers: Node.process_step and a streaming Node.pack
  7  refusals
"""
import ctypes

import numpy as np
import pytest

import dedup_cases as dc
import node_cases as nc
import nydus_gpu
from nydus_gpu import rafs
from test_gpu_dict_fold import _appended, _places, _tables
from test_gpu_dict_retire import _caps, _rows, _same_rows, _table
from test_gpu_node_distill import _node_answers, _once
from test_gpu_node_fold import MODES, _agree, _ask, _k_of, _nfold, _node_model
from test_gpu_node_retire import _owners, _sample_query, _set_owners

pytestmark = pytest.mark.gpu

CS = 0x10000
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
REP = "replicate"


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


def _bytes(tbl):
    if tbl is None or isinstance(tbl, bytes):
        return tbl
    return np.ascontiguousarray(tbl).tobytes()


def _windows(m):
    """The join's window widths for a dict of m rows: 1 (small dicts only), 64, 100,
    m - 1, m, m + 1 and 0 (the default)."""
    ws = ([1] if m <= 257 else []) + [64, 100, m - 1, m, m + 1]
    return list(dict.fromkeys([w for w in ws if w >= 1] + [0]))


def _plain_ref(plain, rows, q, lens):
    """The queries against a plain Engine's dict of the rows."""
    pd = plain.dict_create(rows)
    try:
        return _ask(plain, pd, q, lens)
    finally:
        plain.set_dict(None)
        pd.release()


def _all_agree(tag, node, d, q, lens, ref):
    try:
        for i, e in enumerate(node.engines):
            _agree(f"{tag} engine {i}", _ask(e, d, q, lens), ref)
    finally:
        for e in node.engines:
            e.set_dict(None)


def _model_agrees(tag, node, rows, tbl, mode, q, lens, ref):
    one = node.dict_create(rows, tbl, mode=MODES[mode])
    try:
        _all_agree(f"{tag} dict_create model", node, one, q, lens, ref)
    finally:
        one.release()


def _info_ok(tag, node, d, rows, mode):
    W, m = len(node.engines), len(rows)
    info = node.dict_info(d)
    assert info["mode"] == MODES[mode], (tag, info["mode"])
    assert (info["parts"], info["entries"]) == (W, m), (tag, info)
    per = [m] * W if mode == REP else [int(x) for x in np.bincount(dc.owner_of(rows["block_id"], W), minlength=W)]
    assert info["part_entries"][:W] == per, (tag, info["part_entries"][:W], per)
    assert len(info["part_entries"]) == 64 and not any(info["part_entries"][W:]), tag
    i0 = d.info()
    assert (i0["entries"], i0["record_capacity"], i0["table_capacity"]) == (m,) + _caps(per[0]), (tag, i0)
    assert not i0["shares_base_storage"], tag


def _holds(tag, node, out, rows, tbl, mode, q=None, lens=None, ref=None):
    """(a), (b) and (c) for one result; `rows` / `tbl` are base's export."""
    got, gtbl = node.dict_export_parts(out)
    _same_rows(got, rows, tag)
    assert gtbl == _bytes(tbl), tag
    assert out.info()["blobs"] >= (int(rows["blob_index"].max()) + 1 if len(rows) else 0), tag
    if ref is not None:
        _all_agree(tag, node, out, q, lens, ref)
    _info_ok(tag, node, out, rows, mode)


def _base_as_it_was(tag, node, base, rows, tbl, mode, q, lens, ref):
    """(d)"""
    got, gtbl = node.dict_export_parts(base)
    _same_rows(got, rows, tag + " base")
    assert gtbl == _bytes(tbl), tag
    _all_agree(tag + " base", node, base, q, lens, ref)
    info = node.dict_info(base)
    assert info["mode"] == MODES[mode] and info["entries"] == len(rows), tag


# ---- 1: sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_sizes_both_directions_every_window(W, m, node_of, plain):
    node = node_of(W)
    rng = np.random.default_rng(31000 + 100 * W + m)
    tbl = _table(2, CS)
    rows = _rows(rng, m, rng.integers(0, 2, m), CS)
    if m:
        rows["blob_index"][-1] = 1
    q, lens = _sample_query(rng, rows, cap=400)
    ref = _plain_ref(plain, rows, q, lens)
    rep = node.dict_create(rows, tbl, mode=MODES[REP])
    _model_agrees(f"W={W} m={m} replicate", node, rows, tbl, REP, q, lens, ref)
    for mode in ("copy", "routed"):
        tag = f"W={W} m={m} {mode}"
        _model_agrees(tag, node, rows, tbl, mode, q, lens, ref)
        out = node.dict_remode(rep, MODES[mode])
        _holds(tag + " split", node, out, rows, tbl, mode, q, lens, ref)
        out.release()
        part = node.dict_create(rows, tbl, mode=MODES[mode])
        widths = _windows(m)
        assert 0 in widths and m + 1 in widths and (1 in widths) == (m <= 257)
        for wr in widths:
            out = node.dict_remode(part, MODES[REP], window_records=wr)
            _holds(f"{tag} join window={wr}", node, out, rows, tbl, REP, q, lens, ref)
            out.release()
        _base_as_it_was(tag, node, part, rows, tbl, mode, q, lens, ref)
        part.release()
    _base_as_it_was(f"W={W} m={m} replicate", node, rep, rows, tbl, REP, q, lens, ref)
    rep.release()
    for e in node.engines:
        e.device_status()


T = 256 * 64  # rows per scan tile of the split: kRetireScanTile keep words of 64


@pytest.mark.parametrize("m", [T - 1, T, T + 1, 2 * T + 1])
def test_scan_tile_edges(m, node_of, plain):
    """The replica's rows end before, at and after the end of a scan tile of the split,
    and a join window ends there."""
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(31900 + m)
    rows = _rows(rng, m, rng.integers(0, 2, m), CS)
    rows["blob_index"][-1] = 1
    q, lens = _sample_query(rng, rows, cap=600)
    ref = _plain_ref(plain, rows, q, lens)
    rep = node.dict_create(rows, mode=MODES[REP])
    part = node.dict_create(rows, mode=MODES["routed"])
    for mode in ("copy", "routed"):
        out = node.dict_remode(rep, MODES[mode])
        _holds(f"m={m} split {mode}", node, out, rows, None, mode, q, lens, ref)
        out.release()
    for wr in (0, T, T - 1, 4096):
        out = node.dict_remode(part, MODES[REP], window_records=wr)
        _holds(f"m={m} join window={wr}", node, out, rows, None, REP, q, lens, ref)
        out.release()
    _base_as_it_was(f"m={m}", node, part, rows, None, "routed", q, lens, ref)
    _base_as_it_was(f"m={m}", node, rep, rows, None, REP, q, lens, ref)
    part.release()
    rep.release()
    for e in node.engines:
        e.device_status()


# ---- 2: owners -----------------------------------------------------------------------------
def _owner_layouts(rng, m, W):
    yield "one_owner", _owners(rng, m, W, "one_owner")
    yield "one_empty", _owners(rng, m, W, "one_empty")
    yield "alternate", np.arange(m) % W
    yield "runs of 64", (np.arange(m) // 64) % W
    yield "runs of 65", (np.arange(m) // 65) % W
    yield "sizes", _owners(rng, m, W, "sizes", 3)


@pytest.mark.parametrize("mode", ["copy", "routed"])
@pytest.mark.parametrize("W", [3, 8])
def test_owner_layouts(W, mode, node_of, plain):
    node = node_of(W)
    rng = np.random.default_rng(32000 + 10 * W + (mode == "routed"))
    m = 65 * W * 3 + 7
    tbl = _table(3, CS)
    for layout, owners in _owner_layouts(rng, m, W):
        tag = f"W={W} {mode} {layout}"
        rows = _set_owners(rng, _rows(rng, m, rng.integers(0, 3, m), CS), owners, W)
        rows["blob_index"][0] = 2
        per = np.bincount(owners, minlength=W)
        if layout == "one_owner":
            assert sorted(per)[:-1] == [0] * (W - 1)
        if layout == "one_empty":
            assert per[W // 2] == 0 and (np.delete(per, W // 2) > 0).all()
        q, lens = _sample_query(rng, rows, cap=600)
        ref = _plain_ref(plain, rows, q, lens)
        rep = node.dict_create(rows, tbl, mode=MODES[REP])
        part = node.dict_create(rows, tbl, mode=MODES[mode])
        _model_agrees(tag, node, rows, tbl, mode, q, lens, ref)
        out = node.dict_remode(rep, MODES[mode])
        _holds(tag + " split", node, out, rows, tbl, mode, q, lens, ref)
        out.release()
        for wr in (0, 64, 65, 100):
            out = node.dict_remode(part, MODES[REP], window_records=wr)
            _holds(f"{tag} join window={wr}", node, out, rows, tbl, REP, q, lens, ref)
            out.release()
        _base_as_it_was(tag, node, part, rows, tbl, mode, q, lens, ref)
        _base_as_it_was(tag, node, rep, rows, tbl, REP, q, lens, ref)
        part.release()
        rep.release()
    for e in node.engines:
        e.device_status()


# ---- 3: first entry wins -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed"])
def test_first_entry_wins_on_crafted_part_tables(mode, node_of, plain):
    """node_cases' dict for W = 3: in every part's own table a tag chain on unequal
    digests (with the repeats it carries, some standing before other members of their
    chain), a chain that wraps, and the 0xFFFFFFFF / 0xFFFFFFFE tag pairs; more repeats
    with another index and blob are appended behind them.  After a split and after a
    join the same row answers every digest: the first in table order."""
    W = 3
    node = node_of(W)
    nd = nc.get_dict(W, "full")
    dd, dsz, db, di, duoff, nb = nd.rows
    rows = np.zeros(len(dsz), rafs.CHUNK_INFO_DTYPE)
    rows["block_id"], rows["uncompressed_size"], rows["blob_index"] = dd, dsz, db
    rows["index"], rows["uncompressed_offset"] = di, duoff
    rows["compressed_offset"] = np.arange(len(rows), dtype=np.uint64) * 4096 + 17
    rows["compressed_size"], rows["flags"] = 4000, 1
    chains, wraps, tagff = (nd.row_classes[k] for k in ("part_tagchain", "part_wrap", "tagff"))
    assert any(min(int(r) for r in g[nc.CHAIN:]) < max(int(r) for r in g[:nc.CHAIN]) for g in chains)
    again = [int(g[3]) for g in chains] + [int(g[0]) for g in wraps] + [int(g[5]) for g in chains] + \
            [int(g[-1]) for g in tagff]
    more = rows[again].copy()
    more["blob_index"] = nc.DUP_BLOB
    more["index"] += 7
    recs = np.concatenate([rows, more])
    q = _once(np.stack([x[1] for x in nd.queries] + [recs["block_id"][r] for r in again]))
    first = {}
    for j, d in enumerate(recs["block_id"]):
        first.setdefault(bytes(d), j)
    assert len(first) < len(recs)  # digests held by several rows
    rep = node.dict_create(recs, mode=MODES[REP])
    part = node.dict_create(recs, mode=MODES[mode])
    assert rep.info()["blobs"] == nb
    split = node.dict_remode(rep, MODES[mode])
    joined = [node.dict_remode(part, MODES[REP], window_records=wr) for wr in (0, 1, 64)]
    for tag, d, md, made in [("split", split, mode, True)] + \
                            [(f"join {i}", j, REP, True) for i, j in enumerate(joined)] + \
                            [("base partitioned", part, mode, False), ("base replicated", rep, REP, False)]:
        _node_answers(f"crafted {mode} {tag}", node, d, recs, q)  # the first row of each digest, by a host scan
        got, gtbl = node.dict_export_parts(d)
        _same_rows(got, recs, f"crafted {mode} {tag}")
        assert gtbl is None
        if made:
            _info_ok(f"crafted {mode} {tag}", node, d, recs, md)
    for h in joined + [split, part, rep]:
        h.release()
    for e in node.engines:
        e.device_status()


# ---- 4: round trips and the same-mode calls ------------------------------------------------
@pytest.mark.parametrize("W", [2, 5])
def test_round_trips_and_same_mode(W, node_of, plain):
    node = node_of(W)
    rng = np.random.default_rng(34000 + W)
    m = 3001
    tbl = _table(4, CS)
    rows = _rows(rng, m, rng.integers(0, 4, m), CS)
    rows["blob_index"][5] = 3
    q, lens = _sample_query(rng, rows, cap=600)
    ref = _plain_ref(plain, rows, q, lens)
    rep = node.dict_create(rows, tbl, mode=MODES[REP])
    for mode, other in (("copy", "routed"), ("routed", "copy")):
        tag = f"W={W} {mode}"
        part = node.dict_create(rows, tbl, mode=MODES[mode])
        # replicated -> partitioned -> replicated
        a = node.dict_remode(rep, MODES[mode])
        b = node.dict_remode(a, MODES[REP], window_records=777)
        _holds(tag + " r -> p", node, a, rows, tbl, mode, q, lens, ref)
        _holds(tag + " r -> p -> r", node, b, rows, tbl, REP, q, lens, ref)
        # partitioned -> replicated -> partitioned
        c = node.dict_remode(part, MODES[REP])
        d = node.dict_remode(c, MODES[other])
        _holds(tag + " p -> r", node, c, rows, tbl, REP, q, lens, ref)
        _holds(tag + " p -> r -> p", node, d, rows, tbl, other, q, lens, ref)
        # the same mode: a compacting copy, with the exchange asked for
        e = node.dict_remode(part, MODES[mode])
        f = node.dict_remode(part, MODES[other])
        g = node.dict_remode(part, nydus_gpu.NODE_DICT_PARTITION)  # no exchange bit: the default, copy
        _holds(tag + " p -> p", node, e, rows, tbl, mode, q, lens, ref)
        _holds(tag + " p -> p, the exchange flipped", node, f, rows, tbl, other, q, lens, ref)
        _holds(tag + " p -> p, the default exchange", node, g, rows, tbl, "copy", q, lens, ref)
        _base_as_it_was(tag, node, part, rows, tbl, mode, q, lens, ref)
        for h in (g, f, e, d, c, b, a, part):
            h.release()
    # replicated -> replicated, exchange bits ignored
    for bits in (0, nydus_gpu.NODE_EXCHANGE_ROUTED, nydus_gpu.NODE_EXCHANGE_COPY):
        r2 = node.dict_remode(rep, nydus_gpu.NODE_DICT_REPLICATE | bits)
        _holds(f"W={W} r -> r bits={bits:#x}", node, r2, rows, tbl, REP, q, lens, ref)
        r2.release()
    _base_as_it_was(f"W={W}", node, rep, rows, tbl, REP, q, lens, ref)
    rep.release()
    for e in node.engines:
        e.device_status()


# ---- 5: handles ----------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [("replicate", "copy"), ("replicate", "routed"), ("copy", "replicate"),
                                     ("routed", "replicate")])
def test_older_handles_and_growth_in_place(src, dst, node_of, plain, tmp_path):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(35000 + 7 * (src == "replicate") + (dst == "routed") + 2 * (src == "routed"))
    t3 = _table(3, CS)
    R1 = _rows(rng, 3000, rng.integers(0, 3, 3000), CS)
    R1["blob_index"][:3] = (0, 1, 2)
    R2 = _rows(rng, 300, rng.integers(0, 2, 300), CS)
    R2["blob_index"][:2] = (0, 1)
    R2["block_id"][:100] = R1["block_id"][5:305:3]  # digests the older handle holds
    b = node.dict_create(R1, t3, mode=MODES[src])
    c = node.dict_retire_parts(b, [])  # room: the extend below appends in place
    x1 = node.dict_extend(c, R2, _table(2, CS))
    assert x1.info()["shares_base_storage"]
    x_rows = _appended(R1, 3, R2)
    x_tbl = _bytes(t3) + _bytes(_table(2, CS))
    q, lens = _sample_query(rng, x_rows, cap=800)
    ref_c, ref_x = _plain_ref(plain, R1, q, lens), _plain_ref(plain, x_rows, q, lens)
    assert ref_c[0].tobytes() != ref_x[0].tobytes()
    # an older handle is remoded with only its own rows, the tip with all of them
    o_c = node.dict_remode(c, MODES[dst], window_records=500)
    o_x = node.dict_remode(x1, MODES[dst], window_records=500)
    _holds(f"{src}->{dst} older handle", node, o_c, R1, t3, dst, q, lens, ref_c)
    _holds(f"{src}->{dst} tip", node, o_x, x_rows, x_tbl, dst, q, lens, ref_x)
    _base_as_it_was(f"{src}->{dst} older", node, c, R1, t3, src, q, lens, ref_c)
    _base_as_it_was(f"{src}->{dst} tip", node, x1, x_rows, x_tbl, src, q, lens, ref_x)
    # after a remode, extends and folds of at most s / 2 rows per part append in place and
    # answer as the model extended the same way
    model = node.dict_create(R1, t3, mode=MODES[dst])
    E = _rows(rng, 150, 0, CS)
    E["block_id"][:20] = R1["block_id"][:20]  # base's rows win
    parts = [_tables(rng, 40, rng.random(40) < 0.5) + (None,) for _ in range(W)]
    pl = _places(rng, sum(_k_of(parts)))
    new_rows, B = _node_model(parts, pl)
    s_part = np.full(W, len(R1)) if dst == REP else np.bincount(dc.owner_of(R1["block_id"], W), minlength=W)
    grown_ids = np.concatenate([E["block_id"], new_rows["block_id"]])
    grown = np.full(W, len(grown_ids)) if dst == REP else np.bincount(dc.owner_of(grown_ids, W), minlength=W)
    assert (grown <= s_part // 2).all(), (grown, s_part)
    cap0 = o_c.info()["record_capacity"]
    e_out, e_mod = node.dict_extend(o_c, E, _table(1, CS)), node.dict_extend(model, E, _table(1, CS))
    assert e_out.info()["shares_base_storage"] == 1 and e_out.info()["record_capacity"] == cap0
    ftbl = rafs.make_blob_table([f"{0xF0 + i:064x}" for i in range(B)], CS)
    g_out, g_mod = _nfold(node, e_out, parts, pl, ftbl), _nfold(node, e_mod, parts, pl, ftbl)
    assert g_out.info()["shares_base_storage"] == 1 and g_out.info()["record_capacity"] == cap0
    g_rows = _appended(_appended(R1, 3, E), 4, new_rows)
    g_tbl = _bytes(t3) + _bytes(_table(1, CS)) + _bytes(ftbl)
    q2, lens2 = _sample_query(rng, g_rows, cap=800)
    ref_g = _plain_ref(plain, g_rows, q2, lens2)
    for name, h in (("remode", g_out), ("model", g_mod)):
        got, gtbl = node.dict_export_parts(h)
        _same_rows(got, g_rows, f"{src}->{dst} grown {name}")
        assert gtbl == g_tbl
        _all_agree(f"{src}->{dst} grown {name}", node, h, q2, lens2, ref_g)
        assert node.dict_info(h)["mode"] == MODES[dst]
    _all_agree(f"{src}->{dst} blind to the growth", node, o_c, q, lens, ref_c)
    # retire, distill and save + open of the result equal those of the model
    for name, fn in (("retire", lambda h: node.dict_retire_parts(h, [1, 4])),
                     ("distill", lambda h: node.dict_distill_parts(h, 1)[0])):
        ra, rb = fn(g_out), fn(g_mod)
        ea, eb = node.dict_export_parts(ra), node.dict_export_parts(rb)
        assert len(ea[0]) < len(g_rows), name
        assert ea[0].tobytes() == eb[0].tobytes() and ea[1] == eb[1], (src, dst, name)
        assert ra.info() == rb.info() and node.dict_info(ra) == node.dict_info(rb), (src, dst, name)
        ra.release()
        rb.release()
    path = str(tmp_path / f"remoded-{src}-{dst}.boot")
    assert node.dict_save(o_x, path)["entries"] == len(x_rows)
    back = node.dict_open(path, MODES[dst])
    got, gtbl = node.dict_export_parts(back)
    _same_rows(got, x_rows, f"{src}->{dst} save and open")
    assert gtbl == x_tbl
    for h in (back, g_mod, g_out, e_mod, e_out, model, o_x, o_c, x1, c, b):
        h.release()
    for e in node.engines:
        e.device_status()


@pytest.mark.parametrize("src,dst", [("replicate", "copy"), ("routed", "replicate")])
def test_placement_rows_blob_tables_and_blob_counts(src, dst, node_of, plain):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(36000 + (src == "routed"))
    # 63 / 64 / 65 blobs, with a table and with the count alone
    for nb in (63, 64, 65):
        rows = _rows(rng, 1200, rng.integers(0, nb, 1200), CS)
        rows["blob_index"][:nb] = np.arange(nb)
        tbl = _table(nb, CS)
        for with_tbl in (True, False):
            tag = f"{src}->{dst} nb={nb} table={with_tbl}"
            base = node.dict_create(rows, tbl if with_tbl else None, mode=MODES[src])
            out = node.dict_remode(base, MODES[dst], window_records=333)
            assert out.info()["blobs"] == base.info()["blobs"] == nb, tag
            assert out._has_blob_table() == with_tbl, tag
            _holds(tag, node, out, rows, tbl if with_tbl else None, dst)
            out.release()
            base.release()
    # a base that keeps no placement rows gives a result that keeps none: a fold with no
    # placements onto an empty dict; the export then carries the documented defaults
    parts = [_tables(rng, 200, rng.random(200) < 0.7) + (None,) for _ in range(W)]
    bare, Bb = _node_model(parts, None)
    assert (bare["compressed_size"] == bare["uncompressed_size"]).all() and not bare["compressed_offset"].any()
    empty = node.dict_create(bare[:0], mode=MODES[src])
    f1 = _nfold(node, empty, parts)
    q, lens = _sample_query(rng, bare, cap=400)
    ref = _plain_ref(plain, bare, q, lens)
    out = node.dict_remode(f1, MODES[dst])
    _holds(f"{src}->{dst} no placement rows", node, out, bare, None, dst, q, lens, ref)
    assert out.info()["blobs"] == f1.info()["blobs"] == Bb
    # ... and one that keeps them gives one that keeps them (the exports compare them)
    pl = _places(rng, sum(_k_of(parts)))
    placed, _ = _node_model(parts, pl)
    assert placed["compressed_offset"].any()
    f2 = _nfold(node, empty, parts, pl)
    out2 = node.dict_remode(f2, MODES[dst])
    _holds(f"{src}->{dst} placement rows", node, out2, placed, None, dst, q, lens, ref)
    # a dict of nothing remodes to a dict of nothing that can grow
    out0 = node.dict_remode(empty, MODES[dst])
    _holds(f"{src}->{dst} empty", node, out0, bare[:0], None, dst)
    grown = node.dict_extend(out0, bare)
    _same_rows(node.dict_export_parts(grown)[0], bare, f"{src}->{dst} empty, extended")
    for h in (grown, out0, out2, f2, out, f1, empty):
        h.release()
    for e in node.engines:
        e.device_status()


# ---- 6: real layers ------------------------------------------------------------------------
def test_step_and_streaming_pack_against_a_split_and_a_joined_dict(oracle):
    """A dict of two real layers' chunk digests (the owners are whatever the digests
    say) among random rows: Node.process_step over both layers and a streaming
    Node.pack of each against a dict that was split, and against one that was joined,
    give the results and streams they give against base -- and what the oracle says."""
    import layers
    import torch
    cs = CS
    rng = np.random.default_rng(37000)
    lay = [layers.edge_tar(chunk=cs), layers.oci_upper_tar_go(2)]
    chs = [oracle.tar_chunks(t, cs) for t in lay]
    digs = [oracle.digest_chunks(t, c, "blake3") for t, c in zip(lay, chs)]

    def recs(dig, length, blob):
        r = _rows(rng, len(dig), blob, cs)
        r["block_id"], r["uncompressed_size"] = dig, length
        return r
    half = len(digs[0]) // 2
    rows = np.concatenate([recs(digs[0][:half], chs[0]["length"][:half], 0),
                           _rows(rng, 2000, rng.integers(0, 4, 2000), cs),
                           recs(digs[1][::2], chs[1]["length"][::2], rng.integers(0, 4, len(digs[1][::2]))),
                           recs(digs[0], chs[0]["length"], 3)])  # later repeats of the first rows: they lose
    tbl = _table(4, cs)
    own = dc.owner_of(rows["block_id"], 2)
    assert 0 < (own == 0).sum() < len(rows)

    def expect(i):
        dec, _ = oracle.dedup(digs[i], chs[i]["length"], rows["block_id"], rows["uncompressed_size"],
                              rows["blob_index"], rows["index"], dict_uoff=rows["uncompressed_offset"])
        return dec

    node = nydus_gpu.Node([0, 0], chunk_size=cs)
    try:
        rep = node.dict_create(rows, tbl, mode=MODES[REP])
        part = node.dict_create(rows, tbl, mode=MODES["copy"])
        split = node.dict_remode(rep, MODES["copy"])
        joined = node.dict_remode(part, MODES[REP], window_records=1000)
        for d in (split, joined):
            assert node.dict_export_parts(d)[0].tobytes() == rows.tobytes()
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

        for name, got, base in (("split", split, rep), ("joined", joined, part)):
            got_step, base_step = step(got), step(base)
            got_pack, base_pack = packs(got), packs(base)
            for i in range(2):
                dec = expect(i)
                for tag, r in (("step", got_step[i]), ("pack", got_pack[i][1])):
                    assert np.array_equal(r["digest"], digs[i]), (name, tag, i)
                    for f in ("kind", "index", "blob_index"):
                        assert np.array_equal(r[f], dec[f]), (name, tag, i, f)
                assert got_step[i].tobytes() == base_step[i].tobytes(), (name, i)
                assert got_pack[i][0].tobytes() == base_pack[i][0].tobytes() == np.ascontiguousarray(chs[i]).tobytes()
                assert got_pack[i][1].tobytes() == base_pack[i][1].tobytes(), (name, i)
                assert got_pack[i][2] == base_pack[i][2], (name, i)
        assert (expect(0)["kind"] == nydus_gpu.DICT).sum() > 0
        for h in (joined, split, part, rep):
            h.release()
    finally:
        node.close()


# ---- 7: refusals ---------------------------------------------------------------------------
def test_refusals(node_of, plain):
    W = 3
    node = node_of(W)
    L = nydus_gpu.lib()
    rng = np.random.default_rng(38000)
    rows = _rows(rng, 900, rng.integers(0, 2, 900), CS)
    rows["blob_index"][0] = 1
    tbl = _table(2, CS)
    q, lens = _sample_query(rng, rows, cap=300)
    ref = _plain_ref(plain, rows, q, lens)
    P, R = nydus_gpu.NODE_DICT_PARTITION, nydus_gpu.NODE_DICT_REPLICATE
    COPY, ROUTED = nydus_gpu.NODE_EXCHANGE_COPY, nydus_gpu.NODE_EXCHANGE_ROUTED

    def raw(nd, d, mode):
        h = ctypes.c_void_p(0xDEAD)
        return L.ngpu_node_dict_remode(nd._h, d._h, mode, None, ctypes.byref(h)), h.value

    def raw_info(nd, d):
        info = nydus_gpu._lib.NgpuNodeDictInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, 528)
        return L.ngpu_node_dict_info_get(nd._h, d._h, ctypes.byref(info)), bytes(info) == bytes(528)

    part = node.dict_create(rows, tbl, mode=MODES["copy"])
    rep = node.dict_create(rows, tbl, mode=MODES[REP])
    for base in (part, rep):
        # a bad mode; both exchange bits, on either mode
        for mode in (2, 3, 0x400, 0x80000000, P | 0x1000, P | COPY | ROUTED, R | COPY | ROUTED):
            assert raw(node, base, mode) == (nydus_gpu.EINVAL, None), hex(mode)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            node.dict_remode(base, P | COPY | ROUTED)
        assert x.value.code == nydus_gpu.EINVAL
    # a plain dict
    pd = plain.dict_create(rows, tbl)
    for mode in (P, R):
        assert raw(node, pd, mode) == (nydus_gpu.EINVAL, None)
    assert raw_info(node, pd) == (nydus_gpu.EINVAL, True)
    pd.release()
    # a dict of another node
    other = nydus_gpu.Node([0, 0], chunk_size=CS)
    try:
        for base in (part, rep):
            for mode in (P, R):
                assert raw(other, base, mode) == (nydus_gpu.EINVAL, None)
            assert raw_info(other, base) == (nydus_gpu.EINVAL, True)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            other.dict_remode(part, R)
        assert x.value.code == nydus_gpu.EINVAL
        with pytest.raises(nydus_gpu.NgpuError) as x:
            other.dict_info(rep)
        assert x.value.code == nydus_gpu.EINVAL
    finally:
        other.close()
    # ngpu_dict_export still refuses the split result, and takes the joined one
    split = node.dict_remode(rep, MODES["routed"])
    joined = node.dict_remode(part, R)
    m, nb = ctypes.c_uint64(0), ctypes.c_uint32(0)
    buf = np.zeros(len(rows), rafs.CHUNK_INFO_DTYPE)
    e0 = node.engines[0]._h
    rc = L.ngpu_dict_export(e0, split._h, buf.ctypes.data_as(ctypes.c_void_p), len(buf), ctypes.byref(m), None, 0,
                            ctypes.byref(nb))
    assert rc == nydus_gpu.EUNSUPP and (m.value, nb.value) == (len(rows), 2)
    old, otbl = node.dict_export(joined)
    assert old.tobytes() == rows.tobytes() and otbl == _bytes(tbl)
    # ... and after all of the above both bases answer and remode as before
    _holds("split after the refusals", node, split, rows, tbl, "routed", q, lens, ref)
    _holds("joined after the refusals", node, joined, rows, tbl, REP, q, lens, ref)
    _base_as_it_was("refusals", node, part, rows, tbl, "copy", q, lens, ref)
    _base_as_it_was("refusals", node, rep, rows, tbl, REP, q, lens, ref)
    for h in (joined, split, rep, part):
        h.release()
    for e in node.engines:
        e.device_status()
