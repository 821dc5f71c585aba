"""Node dict fold (ngpu_node_dict_fold, csrc/node.hip + csrc/node_fold.hip) on the
GPU, on nodes that list device 0 W times.

The expectation is what the header defines: ngpu_node_dict_extend over the
concatenated host rows -- test_gpu_dict_fold._model per part, part 0 first, blob
ranks running on across the parts (_node_model).  A replicated dict is compared
through Node.dict_export, byte for byte, three ways: the fold, Node.dict_extend of
the model rows, and the model rows appended to the base's export.  A partitioned
dict cannot be exported, so the fold handle is asked through the product path --
node.engines[i].set_dict(d), then ngpu_dedup_device over supplied digests, on
every engine -- and every field of every answer and every stats field must equal
those of the Node.dict_extend handle, of a Node.dict_create of all rows and of a
plain Engine dict of the same rows.

  1  replicated: sizes at which a wave, a keep word, a tile or a scan tile ends,
     every NEW pattern; the first fold forks, a second one appends in place
  2  partitioned, copy and routed: crafted digests (both sides of every owner
     boundary, one owner takes everything, owners without a row, a part with
     n == 0, a digest NEW in two parts, a digest of the base), k per part at the
     sizes where a wave, a split tile and a scan tile end
  3  layers across parts, blob counts and blob-table rows
  4  older handles stay blind to in-place node folds
  5  placements kept, defaulted and refused; retained Packs against the handle
  6  refusals in a part j > 0 leave every part as it was
  7  real layers through Node.process_step, folded, the next step against the result
"""
import io

import numpy as np
import pytest

import node_cases as nc
import nydus_gpu
from nydus_gpu import rafs
from test_gpu_dict_fold import (CS, DICT, DIGESTED, NEW, T, _appended, _cuts, _dedup, _dev, _fork_caps, _model,
                                _patterns, _places, _same_rows, _tables)

pytestmark = pytest.mark.gpu

MODES = {"copy": nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY,
         "routed": nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_ROUTED,
         "replicate": nydus_gpu.NODE_DICT_REPLICATE}
PART_N = [0, 1, 63, 64, 65, 255, 256, 257, 16385]
PART_K = [257, 1025, 1, 63, 64, 65, 255, 256, 1023, 1024]


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


def _base_rows(rng, m, nb=2):
    r = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
    r["block_id"] = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    r["uncompressed_size"] = CS
    r["blob_index"] = rng.integers(0, nb, m)
    if m:
        r["blob_index"][0] = nb - 1
    r["index"] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    r["uncompressed_offset"] = rng.integers(0, 1 << 44, m, dtype=np.uint64)
    r["compressed_offset"] = rng.integers(0, 1 << 44, m, dtype=np.uint64)
    r["compressed_size"] = rng.integers(1, 1 << 16, m)
    r["flags"] = rng.integers(0, 2, m)
    return r


def _k_of(parts):
    return [0 if p is None else int((p[0]["kind"] == NEW).sum()) for p in parts]


def _node_model(parts, placements=None):
    """parts: (res, ch, first or None) per node device, None = a part with n == 0.
    -> (the concatenated 80-B rows, b over all parts)."""
    rows, B, at = [], 0, 0
    for p, k in zip(parts, _k_of(parts)):
        if p is None:
            continue
        r, b = _model(p[0], p[1], p[2], None if placements is None else placements[at:at + k])
        r["blob_index"] += B
        rows.append(r)
        B += b
        at += k
    return (np.concatenate(rows) if rows else np.zeros(0, rafs.CHUNK_INFO_DTYPE)), B


def _upload(parts):
    """-> (Node.dict_fold's part dicts, the tensors that must stay alive)."""
    import torch
    args, keep = [], []
    for p in parts:
        if p is None:
            args.append({"n": 0})
            continue
        res, ch, first = p
        t = [_dev(res), _dev(ch)] + ([] if first is None else [_dev(np.asarray(first, np.uint64))])
        keep.append(t)
        a = {"d_results": t[0].data_ptr(), "d_chunks": t[1].data_ptr(), "n": len(res)}
        if first is not None:
            a["d_layer_first"], a["n_layers"] = t[2].data_ptr(), len(first) - 1
        args.append(a)
    torch.cuda.synchronize()
    return args, keep


def _nfold(node, base, parts, placements=None, blobs=None):
    args, keep = _upload(parts)
    return node.dict_fold(base, args, placements=placements, blobs=blobs)


def _ask(eng, d, q, lens):
    _, _, host, st = _dedup(eng, d, q, lens)
    return host, st


def _agree(tag, got, ref):
    (a, sa), (b, sb) = got, ref
    for f in ("kind", "ref", "index", "blob_index", "dict_blob", "uncompressed_offset"):
        bad = np.flatnonzero(a[f] != b[f])
        assert not len(bad), f"{tag}: {f} differs at {len(bad)} chunks, first {bad[0]}: {a[f][bad[0]]} vs {b[f][bad[0]]}"
    assert a.tobytes() == b.tobytes(), tag
    assert sa == sb, (tag, sa, sb)


def _query(rng, rows, extra=()):
    """Every row's digest at its size, the extra digests and fresh misses, shuffled."""
    miss = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    q = np.concatenate([rows["block_id"], miss] + [np.asarray(e, np.uint8).reshape(-1, 32) for e in extra])
    lens = np.full(len(q), CS, np.uint32)
    lens[:len(rows)] = np.where(rows["uncompressed_size"] == 0, CS, rows["uncompressed_size"])
    order = rng.permutation(len(q))
    return np.ascontiguousarray(q[order]), lens[order]


def _check_handles(tag, node, plain, rows, q, lens, handles, mode):
    """Every handle, on every engine of the node, answers as a plain Engine dict of
    `rows` and as a node dict created from them in one go."""
    pd = plain.dict_create(rows)
    one = node.dict_create(rows, mode=MODES[mode])
    try:
        ref = _ask(plain, pd, q, lens)
        assert int((ref[0]["kind"] == DICT).sum()) >= len(rows)  # every row answers for its own digest
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


# ---- 1: replicated, three ways through the export ---------------------------------------
@pytest.mark.parametrize("W", [2, 3])
def test_replicated_sizes_and_patterns_three_ways(W, node_of):
    node = node_of(W)
    rng = np.random.default_rng(100 + W)
    m0 = 100
    rows0 = _base_rows(rng, m0, 1)
    base = node.dict_create(rows0, mode=MODES["replicate"])
    seen = set()
    for pi, name in enumerate(("all", "none", "every other", "first", "last", "random 30%")):
        parts = []
        for i in range(W):
            n = PART_N[(pi * W + i) % len(PART_N)]
            seen.add(n)
            new = dict(_patterns(n, rng))[name] if n else None
            parts.append(None if n == 0 and i % 2 else _tables(rng, n, new if n else np.zeros(0, bool)) + (None,))
        K = sum(_k_of(parts))
        pl = _places(rng, K)
        rows, B = _node_model(parts, pl)
        assert len(rows) == K and B == sum(k > 0 for k in _k_of(parts))
        f1 = _nfold(node, base, parts, pl)
        f2 = _nfold(node, f1, parts, pl)
        x1 = node.dict_extend(base, rows)
        x2 = node.dict_extend(x1, rows)
        exp1 = _appended(rows0, 1, rows)
        exp2 = _appended(exp1, 1 + B, rows)
        for tag, f, x, exp, nb in (("fork", f1, x1, exp1, 1 + B), ("share", f2, x2, exp2, 1 + 2 * B)):
            got, gtbl = node.dict_export(f)
            via, _ = node.dict_export(x)
            _same_rows(got, exp, f"W={W} {name} {tag} fold vs model")
            _same_rows(via, exp, f"W={W} {name} {tag} extend vs model")
            assert gtbl is None
            assert f.info() == x.info(), (name, tag, f.info(), x.info())
            assert (f.info()["entries"], f.info()["blobs"]) == (len(exp), nb)
        i1, i2 = f1.info(), f2.info()
        if K:
            assert (i1["record_capacity"], i1["table_capacity"]) == _fork_caps(m0, K), (name, i1)
            assert not i1["shares_base_storage"] and i2["shares_base_storage"], name
        else:  # a handle equal to base
            assert i1["entries"] == m0 and i1["record_capacity"] == m0
        _same_rows(node.dict_export(base)[0], rows0, f"W={W} {name} base")
        for h in (f1, f2, x1, x2):
            h.release()
    assert seen == set(PART_N)
    base.release()
    for e in node.engines:
        e.device_status()


# ---- 2: partitioned, crafted digests ------------------------------------------------------
def _set_prefix(d, p):
    d[0], d[1] = p >> 8, p & 0xFF


def _crafted_steps(rng, W, rows0):
    """The chain of folds of the partitioned test: a list of steps, each a list of W
    parts.  -> (steps, notes): notes name the digests whose answer is asserted."""
    slots = [PART_K[j:j + W] for j in range(0, len(PART_K), W)]
    steps, notes = [], {}
    for s, ks in enumerate(slots):
        parts = []
        for i in range(W):
            k = ks[i] if i < len(ks) else 0
            if k == 0:
                parts.append(None)
                continue
            n = k + k // 3 + 2
            new = np.zeros(n, bool)
            new[rng.choice(n, k, replace=False)] = True
            parts.append(_tables(rng, n, new) + (None,))
        steps.append(parts)
    # step 0: boundary prefixes on both sides of every owner boundary, 0x0000 and 0xFFFF
    big = [i for i, p in enumerate(steps[0]) if p is not None and _k_of([p])[0] >= 64]
    assert len(big) >= 2
    prefixes = sorted({0, 0xFFFF} | {x for b in nc.boundaries(W) for x in (b - 1, b)})
    cursor = {i: iter(np.flatnonzero(steps[0][i][0]["kind"] == NEW)) for i in big}
    for j, p in enumerate(prefixes):
        i = big[j % len(big)]
        _set_prefix(steps[0][i][0]["digest"][next(cursor[i])], p)
    notes["prefixes"] = prefixes
    # the same digest NEW in two parts (same length): the lower part's row answers
    a, b = big[0], big[1]
    ca, cb = next(cursor[a]), next(cursor[b])
    steps[0][b][0]["digest"][cb] = steps[0][a][0]["digest"][ca]
    steps[0][a][1]["length"][ca] = steps[0][b][1]["length"][cb] = CS
    assert steps[0][a][0]["index"][ca] != steps[0][b][0]["index"][cb]
    notes["twice"] = (steps[0][a][0]["digest"][ca].copy(), int(steps[0][a][0]["index"][ca]))
    # a digest the base already holds: the base answers
    cc = next(cursor[b])
    steps[0][b][0]["digest"][cc] = rows0["block_id"][7]
    steps[0][b][1]["length"][cc] = CS
    notes["in_base"] = (rows0["block_id"][7].copy(), int(rows0["index"][7]))
    # a step whose every NEW chunk belongs to owner W - 1 (the others get no row);
    # part 0 has n == 0
    lo, hi = nc.prefix_range(W, W - 1)
    parts = [None]
    for i in range(1, W):
        n = 70 + i
        res, ch = _tables(rng, n, rng.random(n) < 0.7)
        pre = rng.integers(lo, hi + 1, n)
        res["digest"][:, 0], res["digest"][:, 1] = pre >> 8, pre & 0xFF
        parts.append((res, ch, None))
    steps.append(parts)
    return steps, notes


@pytest.mark.parametrize("W,mode", [(W, m) for W in (2, 3, 5, 8) for m in ("copy", "routed")],
                         ids=[f"W{W}-{m}" for W in (2, 3, 5, 8) for m in ("copy", "routed")])
def test_partitioned_crafted_chain_against_three_references(W, mode, node_of, plain):
    node = node_of(W)
    rng = np.random.default_rng(200 + W)
    m0 = 200
    rows0 = _base_rows(rng, m0)
    steps, notes = _crafted_steps(rng, W, rows0)
    assert sorted(k for parts in steps[:-1] for k in _k_of(parts) if k) == sorted(PART_K)
    base = node.dict_create(rows0, mode=MODES[mode])
    f, x, rows, nb = base, base, rows0, 2
    held = []
    try:
        for s, parts in enumerate(steps):
            K = sum(_k_of(parts))
            pl = _places(rng, K)
            new_rows, B = _node_model(parts, pl)
            f, x = _nfold(node, f, parts, pl), node.dict_extend(x, new_rows)
            held += [f, x]
            rows = _appended(rows, nb, new_rows)
            nb += B
            assert f.entries == x.entries == len(rows) and f.info() == x.info(), (s, f.info(), x.info())
            assert f.info()["blobs"] == nb
            if s == 0:
                assert not f.info()["shares_base_storage"]
                own = nc.dc.owner_of(new_rows["block_id"], W)
                assert sorted(set(own.tolist())) == list(range(W))
            if s in (0, len(steps) - 1):
                fresh = [np.frombuffer(rng.bytes(32), np.uint8).copy() for _ in notes["prefixes"]]
                for d, p in zip(fresh, notes["prefixes"]):
                    _set_prefix(d, p)
                q, lens = _query(rng, rows, [np.stack(fresh)])
                ref = _check_handles(f"W{W} {mode} step {s}", node, plain, rows, q, lens,
                                     {"fold": f, "extend": x}, mode)[0]
                for what, (dg, index) in (("twice", notes["twice"]), ("in_base", notes["in_base"])):
                    at = np.flatnonzero((q == dg).all(axis=1))
                    assert len(at) and (ref["kind"][at[0]] == DICT) and ref["index"][at[0]] == index, what
                    if what == "in_base":
                        assert ref["ref"][at[0]] == 7
        own = nc.dc.owner_of(_node_model(steps[-1])[0]["block_id"], W)
        assert (own == W - 1).all()
    finally:
        for h in held:
            h.release()
        base.release()
        for e in node.engines:
            e.device_status()


# ---- 3: layers ----------------------------------------------------------------------------
@pytest.mark.parametrize("W,mode", [(3, "replicate"), (2, "copy")], ids=["W3-replicate", "W2-copy"])
def test_layers_across_parts_blob_ranks_and_tables(W, mode, node_of, plain):
    """Part 0: 64 layers with empty ones and every third without a NEW chunk; part 1:
    one layer without a NEW chunk (b = 0); part 2: five layers, the first and the
    last empty.  The base has a blob table, so the call brings b rows in global order."""
    node = node_of(W)
    rng = np.random.default_rng(300 + W)

    def layered(n, L, barren_every=3):
        first = _cuts(rng, n, L)
        layer = np.searchsorted(first[1:], np.arange(n), side="right")
        barren = np.arange(L) % barren_every == 2
        res, ch = _tables(rng, n, (rng.random(n) < 0.4) & ~barren[layer])
        return res, ch, first

    parts = [layered(T + 500, 64), _tables(rng, 300, np.zeros(300, bool)) + (None,), layered(700, 5)][:W]
    if W == 2:
        parts[1] = layered(700, 5)
    rows0 = _base_rows(rng, 50)
    tbl0 = rafs.make_blob_table([f"{i:064x}" for i in range(2)], CS)
    base = node.dict_create(rows0, tbl0, mode=MODES[mode])
    K = sum(_k_of(parts))
    pl = _places(rng, K)
    rows, B = _node_model(parts, pl)
    per_part = [_model(p[0], p[1], p[2])[1] for p in parts]
    assert B == sum(per_part) and per_part[0] > 3 and per_part[-1] >= 2
    assert len(set(rows["blob_index"])) == B == int(rows["blob_index"].max()) + 1
    assert (np.diff(rows["blob_index"].astype(np.int64)) >= 0).all()  # blob ranks run on across the parts
    tbl = rafs.make_blob_table([f"{0xAB00 + i:064x}" for i in range(B)], CS)
    f = _nfold(node, base, parts, pl, tbl)
    x = node.dict_extend(base, rows, tbl)
    try:
        assert f.info() == x.info() and f.info()["blobs"] == 2 + B and f._has_blob_table()
        exp = _appended(rows0, 2, rows)
        if mode == "replicate":
            got, gtbl = node.dict_export(f)
            via, vtbl = node.dict_export(x)
            _same_rows(got, exp, "fold vs model")
            _same_rows(via, exp, "extend vs model")
            assert gtbl == vtbl == np.ascontiguousarray(tbl0).tobytes() + np.ascontiguousarray(tbl).tobytes()
        q, lens = _query(rng, exp)
        ref = _check_handles(f"layers W{W} {mode}", node, plain, exp, q, lens, {"fold": f, "extend": x}, mode)[0]
        assert len(set(ref["dict_blob"][ref["kind"] == DICT].tolist())) > B // 2
        for wrong in (B - 1, B + 1):  # n_blobs == b over all parts
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                _nfold(node, base, parts, pl, rafs.make_blob_table([f"{i:064x}" for i in range(wrong)], CS))
            assert ei.value.code == nydus_gpu.EINVAL and "blob table" in str(ei.value)
        with pytest.raises(nydus_gpu.NgpuError) as ei:  # the base has a table, the call brings none
            _nfold(node, base, parts, pl)
        assert ei.value.code == nydus_gpu.EINVAL
    finally:
        for h in (f, x, base):
            h.release()
        for e in node.engines:
            e.device_status()


# ---- 4: older handles ---------------------------------------------------------------------
@pytest.mark.parametrize("W,mode", [(2, "copy"), (3, "routed"), (2, "replicate")],
                         ids=["W2-copy", "W3-routed", "W2-replicate"])
def test_older_handles_stay_blind_after_in_place_node_folds(W, mode, node_of, plain):
    """f1 forks, f2 and f3 append in place behind it on every part.  With f3 alive,
    every handle answers, on every engine, for exactly its own rows."""
    node = node_of(W)
    rng = np.random.default_rng(400 + W)
    rows0 = _base_rows(rng, 200)
    d0 = node.dict_create(rows0, mode=MODES[mode])
    chain, rows, nb = [("d0", d0, rows0)], rows0, 2
    for size in (400, 60, 60):
        parts = [_tables(rng, size, rng.random(size) < 0.8) + (None,) for _ in range(W)]
        pl = _places(rng, sum(_k_of(parts)))
        new_rows, B = _node_model(parts, pl)
        rows = _appended(rows, nb, new_rows)
        nb += B
        chain.append((f"f{len(chain)}", _nfold(node, chain[-1][1], parts, pl), rows))
    try:
        shares = [d.info()["shares_base_storage"] for _, d, _ in chain]
        assert shares == [False, False, True, True], shares
        q, lens = _query(rng, rows)
        hits = []
        for name, d, own_rows in reversed(chain):
            ref = _check_handles(f"blind W{W} {mode} {name}", node, plain, own_rows, q, lens, {name: d}, mode)[0]
            hits.append(int((ref["kind"] == DICT).sum()))
        assert hits[0] > hits[1] > hits[2] > hits[3] > 0, hits
    finally:
        for _, d, _ in chain:
            d.release()
        for e in node.engines:
            e.device_status()


# ---- 5: placements ------------------------------------------------------------------------
def test_placements_kept_defaulted_and_refused(node_of):
    W = 2
    node = node_of(W)
    rng = np.random.default_rng(500)
    parts = [_tables(rng, 300, rng.random(300) < 0.5) + (None,), _tables(rng, 65, np.ones(65, bool)) + (None,)]
    ks = _k_of(parts)
    K = sum(ks)
    pl = _places(rng, K)
    rows0 = _base_rows(rng, 40, 1)
    with_pl = node.dict_create(rows0, mode=MODES["replicate"])
    empty = node.dict_create(np.zeros(0, rafs.CHUNK_INFO_DTYPE), mode=MODES["replicate"])
    rows, B = _node_model(parts, pl)
    rows_np, _ = _node_model(parts)
    held = [with_pl, empty]
    try:
        f = _nfold(node, with_pl, parts, pl)                 # kept: global order, part 0's first
        x = node.dict_extend(with_pl, rows)
        e1, e2 = _nfold(node, empty, parts, pl), _nfold(node, empty, parts)
        held += [f, x, e1, e2]
        _same_rows(node.dict_export(f)[0], _appended(rows0, 1, rows), "placements kept")
        assert node.dict_export(x)[0].tobytes() == node.dict_export(f)[0].tobytes()
        _same_rows(node.dict_export(e1)[0], rows, "empty base, placements")
        got = node.dict_export(e2)[0]                         # defaulted: csize = usize, offset 0, flags 0
        _same_rows(got, rows_np, "empty base, none")
        assert (got["compressed_size"] == got["uncompressed_size"]).all() and not got["flags"].any()
        for base, kw, what in ((with_pl, {}, "the base keeps placements, none given"),
                               (e2, {"placements": pl}, "the base keeps none, some given"),
                               (with_pl, {"placements": pl[:ks[0]]}, "part 0's rows only"),
                               (with_pl, {"placements": pl[:-1]}, "k - 1"),
                               (with_pl, {"placements": np.concatenate([pl, pl[:1]])}, "k + 1"),
                               (empty, {"placements": pl[:1]}, "n_placements != k on an empty base")):
            before = node.dict_export(base)[0].tobytes()
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                _nfold(node, base, parts, **kw)
            assert ei.value.code == nydus_gpu.EINVAL, what
            assert node.dict_export(base)[0].tobytes() == before, what
        none_new = [_tables(rng, 64, np.zeros(64, bool)) + (None,), None]
        for base in (with_pl, e2):                            # k == 0 over all parts: a handle equal to base
            z = _nfold(node, base, none_new)
            z2 = _nfold(node, base, none_new, np.zeros(0, nydus_gpu.DICT_PLACE_DTYPE))
            held += [z, z2]
            assert node.dict_export(z)[0].tobytes() == node.dict_export(z2)[0].tobytes() == \
                node.dict_export(base)[0].tobytes()
            assert z.info()["entries"] == base.entries and z.info()["blobs"] == base.info()["blobs"]
    finally:
        for h in held:
            h.release()
        for e in node.engines:
            e.device_status()


@pytest.mark.parametrize("W,mode", [(2, "copy"), (3, "routed")], ids=["W2-copy", "W3-routed"])
def test_retained_packs_against_the_fold_handle_equal_the_extend_handle(W, mode, node_of, tars):
    """A layer's result table, cut over the parts, folded with placements into a
    partitioned dict: retained Packs of the layer finished against the fold handle
    copy the very dict records (placements included) they copy against the extend
    handle."""
    node = node_of(W)
    rng = np.random.default_rng(550 + W)
    tar = tars["oci_upper"]
    with nydus_gpu.Engine(chunk_size=CS, staging_bytes=4 * CS) as eng:
        ch, out, _ = eng.pack_tar(tar)
    n = len(ch)
    cuts = np.linspace(0, n, W + 1).astype(int)
    parts = [(out[a:b].copy(), ch[a:b].copy(), None) for a, b in zip(cuts[:-1], cuts[1:])]
    K = sum(_k_of(parts))
    assert K > W
    pl = _places(rng, K)
    rows, B = _node_model(parts, pl)
    rows0 = _base_rows(rng, 30)
    base = node.dict_create(rows0, mode=MODES[mode])
    f = _nfold(node, base, parts, pl)
    x = node.dict_extend(base, rows)
    try:
        streams = {}
        for name, d in (("fold", f), ("extend", x)):
            ws = [node.pack(d, retain=True) for _ in range(W)]
            for w in ws:
                w.write(tar)
            streams[name] = []
            for w in ws:
                o = io.BytesIO()
                _, res, st, _ = w.finish(o, compressor="none")
                assert st["dict_chunks"] == int((res["kind"] == DICT).sum()) >= K  # (repeats hit too)
                streams[name].append((o.getvalue(), res.tobytes()))
        assert streams["fold"] == streams["extend"]
    finally:
        for h in (f, x, base):
            h.release()
        for e in node.engines:
            e.device_status()


# ---- 6: refusals --------------------------------------------------------------------------
def test_refusals_in_a_later_part_leave_every_part_a_tip(node_of, plain):
    """The refused table sits in part 1 or 2, so parts before it were valid and would
    have been reserved by a call that decided part by part.  After each refusal
    every engine still answers as before, and a valid fold right after appends in
    place (info() reports part 0; the other parts' rows are checked by their
    answers and entry counts)."""
    W, mode = 3, "copy"
    node = node_of(W)
    rng = np.random.default_rng(600)
    rows0 = _base_rows(rng, 300)
    base = node.dict_create(rows0, mode=MODES[mode])
    seed = [_tables(rng, 400, np.ones(400, bool)) + (None,) for _ in range(W)]
    pls = _places(rng, 1200)
    rows_tip = _appended(rows0, 2, _node_model(seed, pls)[0])
    n = 500
    good = [(*_tables(rng, n, rng.random(n) < 0.3), [0, 100, 100, n]) for _ in range(W)]
    Kg = sum(_k_of(good))
    q, lens = _query(rng, rows_tip, [np.concatenate([p[0]["digest"] for p in good])])
    held = [base]
    try:
        tip = _nfold(node, base, seed, pls)  # a tip with room on every part
        held.append(tip)
        pd = plain.dict_create(rows_tip)
        held.append(pd)
        ref = _ask(plain, pd, q, lens)
        plain.set_dict(None)

        def refused(parts, needles, pl=None):
            nonlocal tip
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                _nfold(node, tip, parts, _places(rng, sum(_k_of(parts))) if pl is None else pl)
            assert ei.value.code == nydus_gpu.EINVAL, str(ei.value)
            for s in needles:
                assert s in str(ei.value), (s, str(ei.value))
            for i, e in enumerate(node.engines):
                _agree(f"after a refusal, engine {i}", _ask(e, tip, q, lens), ref)
                e.set_dict(None)
            ok = [_tables(rng, 30, np.ones(30, bool)) + (None,) for _ in range(W)]
            nxt = _nfold(node, tip, ok, _places(rng, 30 * W))  # a valid fold right after: in place
            assert nxt.info()["shares_base_storage"] and nxt.entries == tip.entries + 30 * W
            nxt.release()
            fresh = _nfold(node, base, seed, pls)  # (the slots stay dead on the storage)
            tip.release()
            held.remove(tip)
            tip = fresh
            held.append(tip)

        for j, kind, at in ((1, DIGESTED, 0), (2, 7, n - 1), (1, 4, n // 2)):
            bad = [(p[0].copy(), p[1], p[2]) for p in good]
            bad[j][0]["kind"][at] = kind
            refused(bad, (f"part {j}", f"chunk {at} "))
        new_at = int(np.flatnonzero(good[2][0]["kind"] == NEW)[5])
        for length in (0, CS + 1):
            bad = [(p[0], p[1].copy(), p[2]) for p in good]
            bad[2][1]["length"][new_at] = length
            refused(bad, ("part 2", f"NEW chunk {new_at} "))
        for cuts in ([0, 100, 99, n], [0, 100, 100, n - 1], [1, 100, 100, n], [0, n + 5, n + 5, n]):
            bad = list(good)
            bad[1] = (good[1][0], good[1][1], cuts)
            refused(bad, ("part 1", "layer_first"), _places(rng, Kg))
        # the wrong number of parts, a plain dict, a dict of another node, the engine call
        for parts in (good[:2], good + good[:1]):
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                _nfold(node, tip, parts, _places(rng, sum(_k_of(parts))))
            assert ei.value.code == nydus_gpu.EINVAL and "parts" in str(ei.value)
        with pytest.raises(nydus_gpu.NgpuError) as ei:
            _nfold(node, pd, good, _places(rng, Kg))
        assert ei.value.code == nydus_gpu.EINVAL and "not a node dict" in str(ei.value)
        args, keep = _upload(good[:1])
        v = nydus_gpu.ChunkDict(tip._h, node.engines[0])  # ngpu_dict_fold keeps refusing node dicts
        try:
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                v.fold(args[0]["d_results"], args[0]["d_chunks"], n, placements=_places(rng, _k_of(good[:1])[0]))
            assert ei.value.code == nydus_gpu.EINVAL
        finally:
            v._h = None
        with nydus_gpu.Node([0, 0], chunk_size=CS, staging_bytes=4 * CS) as other:
            with pytest.raises(nydus_gpu.NgpuError) as ei:
                other.dict_fold(tip, _upload(good[:2])[0], placements=_places(rng, sum(_k_of(good[:2]))))
            assert ei.value.code == nydus_gpu.EINVAL
        last = _nfold(node, tip, good, _places(rng, Kg))  # and the tip is still a tip
        held.append(last)
        assert last.info()["shares_base_storage"] and last.entries == tip.entries + Kg
    finally:
        for h in held:
            h.release()
        for e in node.engines:
            e.device_status()


# ---- 7: end to end ------------------------------------------------------------------------
def _layer(rng, total):
    data = bytearray(rng.integers(0, 256, total, dtype=np.uint8).tobytes())
    chunks, off = [], 0
    while True:
        ln = int(rng.integers(1, CS + 1)) if rng.random() < 0.5 else CS
        if off + ln > total:
            break
        chunks.append((off, ln, len(chunks), 0))
        off = (off + ln + 511) // 512 * 512
    return data, np.array(chunks, dtype=nydus_gpu.CHUNK_DTYPE)


def _repeat_chunks(rng, data, ch, src_data, src_ch, count):
    """`count` chunks of (data, ch) become copies of chunks of the source layer."""
    for b in rng.choice(len(ch), min(count, len(ch)), replace=False):
        a = int(rng.integers(0, len(src_ch)))
        ln = int(src_ch["length"][a])
        if ln <= int(ch["length"][b]):
            ch["length"][b] = ln
            so, do = int(src_ch["offset"][a]), int(ch["offset"][b])
            data[do:do + ln] = src_data[so:so + ln]


@pytest.mark.parametrize("W,mode", [(W, m) for W in (2, 3) for m in ("copy", "replicate")],
                         ids=[f"W{W}-{m}" for W in (2, 3) for m in ("copy", "replicate")])
def test_process_step_fold_next_step_equals_the_oracle(W, mode, node_of, oracle):
    """C4's loop: a step's layers (peer copies, not RCCL) are folded into the node
    dict, the next step's layers dedup against the result; every decision equals the
    oracle's with the concatenated dict."""
    import torch
    node = node_of(W)
    rng = np.random.default_rng(700 + W)

    def expect(dig, ch, recs):
        return oracle.dedup(dig, ch["length"], recs["block_id"], recs["uncompressed_size"], recs["blob_index"],
                            recs["index"], dict_uoff=recs["uncompressed_offset"])[0]

    def step(d, layers, recs):
        """layers: per part a list of (data, chunks) -> (fold parts, host tables)."""
        args, keep, host = [], [], []
        for ls in layers:
            data = b"".join(bytes(x[0]) for x in ls)
            chs, first, at = [], [0], 0
            for x in ls:
                c = x[1].copy()
                c["offset"] += at
                at += len(x[0])
                chs.append(c)
                first.append(first[-1] + len(c))
            ch = np.concatenate(chs)
            t = (_dev(np.frombuffer(data, np.uint8)), _dev(ch), _dev(np.asarray(first, np.uint64)),
                 torch.zeros(len(ch) * 64, dtype=torch.uint8, device="cuda"))
            keep.append(t)
            args.append({"d_data": t[0].data_ptr(), "len": len(data), "d_chunks": t[1].data_ptr(), "n": len(ch),
                         "d_out": t[3].data_ptr(), "d_layer_first": t[2].data_ptr(), "n_layers": len(ls)})
            host.append((data, ch, first))
        torch.cuda.synchronize()
        node.process_step(d, args)
        torch.cuda.synchronize()
        tables = []
        for (data, ch, first), t in zip(host, keep):
            got = t[3].cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
            for a, b in zip(first[:-1], first[1:]):  # every layer on its own under the whole dict
                dig = oracle.digest_chunks(data, ch[a:b].view(oracle.CHUNK_DTYPE), "blake3")
                dec = expect(dig, ch[a:b], recs)
                assert np.array_equal(got["digest"][a:b], dig)
                assert np.array_equal(got["kind"][a:b], dec["kind"])
                hit = dec["kind"] == DICT
                for f in ("index", "ref", "blob_index", "uncompressed_offset"):
                    assert np.array_equal(got[f][a:b][hit], dec[f][hit]), f
            tables.append((got.copy(), ch, first))
        return args, keep, tables

    l1 = [[_layer(rng, 1 << 20) for _ in range(2 if i == 0 else 1)] for i in range(W)]
    l2 = [[_layer(rng, 1 << 20)] for _ in range(W)]
    for i in range(W):  # the next step repeats chunks of every part of the first
        for j in range(W):
            _repeat_chunks(rng, l2[i][0][0], l2[i][0][1], l1[j][0][0], l1[j][0][1], 4)
    rows0 = _base_rows(rng, 100)
    dig0 = oracle.digest_chunks(l1[0][0][0], l1[0][0][1].view(oracle.CHUNK_DTYPE), "blake3")
    rows0["block_id"][:5] = dig0[:5]
    rows0["uncompressed_size"][:5] = l1[0][0][1]["length"][:5]
    base = node.dict_create(rows0, mode=MODES[mode])
    held = [base]
    try:
        args, keep, tables = step(base, l1, rows0)
        K = sum(_k_of(tables))
        pl = _places(rng, K)
        f = node.dict_fold(base, args, placements=pl)
        held.append(f)
        new_rows, B = _node_model(tables, pl)
        assert B == W + 1 and f.info()["blobs"] == 2 + B and f.entries == 100 + K
        allrows = _appended(rows0, 2, new_rows)
        _, _, t2 = step(f, l2, allrows)
        assert sum(int((t[0]["kind"] == DICT).sum()) for t in t2) >= W  # the repeats hit the folded rows
        x = node.dict_extend(base, new_rows)
        held.append(x)
        assert f.info() == x.info()
    finally:
        for h in held:
            h.release()
        for e in node.engines:
            e.device_status()
