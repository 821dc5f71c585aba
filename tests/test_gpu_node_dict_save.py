"""Dict save for node dicts (ngpu_node_dict_save, csrc/dict_save.hip + csrc/node.hip)
on the GPU, on nodes that list device 0 W times, in both dict modes.

A partitioned dict's rows lie on its parts in ascending global id order; a window of
ids is one slice per part, and the scatter kernel puts every row at its id.  The
expectation is the plain call's: the bytes rafs.write_v6_bootstrap gives for the
rows in global table order, equal to ngpu_dict_save of a plain dict of those rows.

  1  node_cases' crafted rows: parts that own no row, rows that all go to one owner,
     windows of 7 / 64 / m records that cut inside owner runs
  2  after Node.dict_extend, Node.dict_fold and Node.dict_retire_parts, and a range
     save over the extend
  3  the replicated mode through both calls; a plain dict through the node call
"""
import io

import numpy as np
import pytest

import dedup_cases as dc
import node_cases as nc
import nydus_gpu
from nydus_gpu import rafs
from test_gpu_dict_fold import _appended, _places, _tables
from test_gpu_dict_retire import _filtered, _rows, _same_rows, _table_rows
from test_gpu_node_fold import MODES, _k_of, _nfold, _node_model

pytestmark = pytest.mark.gpu

CS = 0x10000
PART_N = [257, 64, 1025, 1, 63, 300, 65, 129]


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


def _table(nb, first=0):
    return rafs.make_blob_table([f"{i:064x}" for i in range(first, first + nb)], CS)


def _expect(rows, tbl=None):
    return rafs.write_v6_bootstrap(rows, CS, flags=0x4, blobs=tbl)


def _nsave(node, d, **kw):
    out = io.BytesIO()
    info = node.dict_save(d, out, **kw)
    data = out.getvalue()
    assert info["bytes"] == len(data)
    return data, info


def _psave(d, **kw):
    out = io.BytesIO()
    d.save(out, **kw)
    return out.getvalue()


def _records(nd, rng):
    """node_cases rows as 80-B records, each with a placement of its own."""
    dd, ds, db, di, duoff, _ = nd.rows
    r = np.zeros(nd.m, rafs.CHUNK_INFO_DTYPE)
    r["block_id"], r["uncompressed_size"], r["blob_index"], r["index"], r["uncompressed_offset"] = dd, ds, db, di, duoff
    r["compressed_offset"] = rng.integers(0, 1 << 44, nd.m, dtype=np.uint64)
    r["compressed_size"] = rng.integers(1, 1 << 16, nd.m)
    r["flags"] = rng.integers(0, 2, nd.m)
    return r


# ---- 1: crafted rows -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", nc.VARIANTS)
@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_crafted_rows_every_window_cut(W, variant, node_of, plain):
    node = node_of(W)
    nd = nc.get_dict(W, variant)
    rng = np.random.default_rng(W)
    rows, tbl = _records(nd, rng), _table(nc.N_BLOBS)
    m = len(rows)
    if variant == "one_empty":
        assert nd.pm[W // 2] == 0
    if variant == "one_owner":
        assert nd.pm[W - 1] == m
    exp = _expect(rows, tbl)
    pd = plain.dict_create(rows, tbl)
    assert _psave(pd) == exp
    for mode in ("copy", "routed", "replicate"):
        d = node.dict_create(rows, tbl, mode=MODES[mode])
        for wr in (7, 64, m, 0):
            got, info = _nsave(node, d, window_records=wr)
            _same_rows(rafs.read_v6(got)["chunks"], rows, f"{mode} wr={wr}")
            assert got == exp, (mode, wr)
            assert info["windows"] == -(-m // (wr or m)) and (info["entries"], info["blobs"]) == (m, nc.N_BLOBS)
        assert _nsave(node, d, no_blob_table=True)[0] == _expect(rows, None)
        # an empty dict grown by an extend, without a blob table: refused unless the flag is set
        bare = node.dict_create(rows[:0], mode=MODES[mode])
        assert _nsave(node, bare)[0] == _expect(rows[:0], None)
        grown = node.dict_extend(bare, rows)
        with pytest.raises(nydus_gpu.NgpuError) as x:
            _nsave(node, grown)
        assert x.value.code == nydus_gpu.EINVAL and "NGPU_DICT_SAVE_NO_BLOB_TABLE" in str(x.value)
        assert _nsave(node, grown, no_blob_table=True, window_records=7)[0] == _expect(rows, None)
        for h in (grown, bare, d):
            h.release()
    pd.release()


# ---- 2: after extend, fold and retire; a range save ----------------------------------------------
@pytest.mark.parametrize("mode", ["copy", "routed", "replicate"])
@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_after_extend_fold_and_retire(W, mode, node_of, plain):
    node = node_of(W)
    rng = np.random.default_rng(10 * W + len(mode))
    rows, tbl = _rows(rng, 2000, rng.integers(0, 2, 2000), CS), _table(2)
    rows["blob_index"][0] = 1
    more, mtbl = _rows(rng, 700, 0, CS), _table(1, first=10)
    d = node.dict_create(rows, tbl, mode=MODES[mode])
    x = node.dict_extend(d, more, mtbl)
    x_rows, x_tbl = _appended(rows, 2, more), np.concatenate([tbl, mtbl])
    parts = [_tables(rng, n, rng.random(n) < 0.6) + (None,) for n in PART_N[:W]]
    pl = _places(rng, sum(_k_of(parts)))
    frows, B = _node_model(parts, pl)
    ftbl = _table(B, first=20)
    f = _nfold(node, x, parts, pl, blobs=ftbl)
    f_rows, f_tbl = _appended(x_rows, 3, frows), np.concatenate([x_tbl, ftbl])
    r = node.dict_retire_parts(f, [1])
    r_rows, kept = _filtered(f_rows, [1], 3 + B)
    r_tbl = np.frombuffer(_table_rows(f_tbl, kept), rafs.BLOB_DTYPE)
    for tag, h, hrows, htbl in (("create", d, rows, tbl), ("extend", x, x_rows, x_tbl), ("fold", f, f_rows, f_tbl),
                                ("retire", r, r_rows, r_tbl)):
        exp = _expect(hrows, htbl)
        for wr in (64, 1000, 0):
            got, info = _nsave(node, h, window_records=wr)
            _same_rows(rafs.read_v6(got)["chunks"], hrows, f"{tag} wr={wr}")
            assert got == exp, (tag, wr)
        erows, etbl = node.dict_export_parts(h)
        assert erows.tobytes() == hrows.tobytes() and etbl == np.ascontiguousarray(htbl).tobytes()
    pd = plain.dict_create(r_rows, r_tbl)
    assert _psave(pd) == _expect(r_rows, r_tbl)
    pd.release()
    # a range save over the extend, and over extend + fold
    for h, hrows, htbl in ((x, x_rows, x_tbl), (f, f_rows, f_tbl)):
        tail = hrows[len(rows):].copy()
        tail["blob_index"] -= 2
        for wr in (0, 64):
            got, info = _nsave(node, h, first_entry=len(rows), first_blob=2, window_records=wr)
            assert got == _expect(tail, htbl[2:]), wr
            assert (info["entries"], info["blobs"]) == (len(tail), len(htbl) - 2)
    # the retired dict does not descend from d by extends: refused, naming the entry
    low = np.flatnonzero((np.arange(len(r_rows)) >= 5) & (r_rows["blob_index"] < 1))
    with pytest.raises(nydus_gpu.NgpuError) as e:
        _nsave(node, r, first_entry=5, first_blob=1)
    assert e.value.code == nydus_gpu.EINVAL and f"entry {int(low[0])} " in str(e.value)
    for h in (r, f, x, d):
        h.release()


# ---- 3: the replicated mode through both calls; refusals ----------------------------------------
def test_replicated_through_both_calls_and_refusals(node_of, plain):
    W = 3
    node = node_of(W)
    rng = np.random.default_rng(33)
    rows, tbl = _rows(rng, 1500, rng.integers(0, 3, 1500), CS), _table(3)
    rows["blob_index"][-1] = 2
    exp = _expect(rows, tbl)
    rep = node.dict_create(rows, tbl, mode=MODES["replicate"])
    for i, e in enumerate(node.engines):
        assert _psave(rep, engine=e, window_records=100) == exp, i
    assert _nsave(node, rep, window_records=100)[0] == exp
    part = node.dict_create(rows, tbl, mode=MODES["copy"])
    with pytest.raises(nydus_gpu.NgpuError) as x:
        _psave(part, engine=node.engines[1])
    assert x.value.code == nydus_gpu.EUNSUPP and "ngpu_node_dict_save" in str(x.value)
    pd = plain.dict_create(rows, tbl)
    with pytest.raises(nydus_gpu.NgpuError) as x:
        _nsave(node, pd)  # a plain dict is not for the node call
    assert x.value.code == nydus_gpu.EINVAL
    assert _psave(pd) == exp
    for kw in ({"first_entry": len(rows) + 1}, {"first_blob": 4}):
        with pytest.raises(nydus_gpu.NgpuError) as x:
            _nsave(node, part, **kw)
        assert x.value.code == nydus_gpu.EINVAL
    assert dc.owner_of(rows["block_id"], W).max() == W - 1  # (every part owns rows here)
    for h in (pd, part, rep):
        h.release()
