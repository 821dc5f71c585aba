"""The crafted node dict cases (node_cases.py) on the CPU: the oracle equals
the model on every case of the GPU matrix (test_gpu_node_collisions.py), each
class has the property it is named for -- owners, home slots through
dedup_cases.home_slot, the wrap, the boundary sides -- and the builder is
deterministic, so that a later change cannot quietly empty a class."""
import numpy as np
import pytest

import dedup_cases as dc
import node_cases as nc
from test_dedup_cases import DICT, FIELDS, INTRA, NEW, NONE, expect

WS = (2, 3, 5, 8)
DICTS = [(W, v) for W in WS for v in nc.VARIANTS]
LAYERS = [(W, v, n, "mixed") for W, v in DICTS for n in nc.LAYER_N] + \
         [(W, "full", n, k) for W in WS for n in (257, 4097) for k in ("one", "avoid")]


def _first_rows(dd):
    first = {}
    for j in range(len(dd)):
        first.setdefault(bytes(dd[j]), j)
    return first


@pytest.mark.parametrize("W,variant", DICTS, ids=[f"W{W}-{v}" for W, v in DICTS])
def test_dict_classes_hold(W, variant):
    nd = nc.get_dict(W, variant)
    dd, ds, db, di, duoff, n_blobs = nd.rows
    rc, own = nd.row_classes, nd.owners
    assert np.array_equal(own, (dd[:, 0].astype(np.int64) << 8 | dd[:, 1]) * W >> 16)
    populated = {"full": set(range(W)), "one_empty": set(range(W)) - {W // 2}, "one_owner": {W - 1}}[variant]
    assert {o for o in range(W) if nd.pm[o]} == populated
    assert [nd.cap[o] for o in range(W) if o not in populated] == [16] * (W - len(populated))  # dict.m == 0
    assert set(rc) == {"part_tagchain", "part_wrap", "tagff", "boundary", "wildcard", "sizerule", "duprow",
                       "unhit", "plain"}
    first = _first_rows(dd)
    # one chain and one wrapping chain per populated part
    for cls in ("part_tagchain", "part_wrap"):
        assert sorted(int(own[g[0]]) for g in rc[cls]) == sorted(populated)
    for g in rc["part_tagchain"]:
        o = int(own[g[0]])
        mem, rep = g[:nc.CHAIN], g[nc.CHAIN:]
        assert len(mem) >= 6 and len(rep) == 2
        d = dd[mem]
        assert (d[:, :12] == d[0, :12]).all() and len({bytes(x) for x in d}) == len(mem)
        assert (own[g] == o).all() and len(set(dc.home_slot(dd[g], nd.cap[o] - 1).tolist())) == 1
        assert len(set(dc.tag_of(dd[g]).tolist())) == 1
        near = d[0] != d[1]
        assert near[31] and near.sum() == 1
        for r, j in zip(rep, (0, 2)):  # later duplicate rows are never the answer
            assert np.array_equal(dd[r], d[j]) and r > mem[j] and first[bytes(dd[r])] == mem[j]
            assert db[r] != db[mem[j]]
    for g in rc["part_wrap"]:
        o = int(own[g[0]])
        assert len(g) >= 5 and (own[g] == o).all()
        assert (dc.home_slot(dd[g], nd.cap[o] - 1) == nd.cap[o] - 2).all()  # cap - 2, cap - 1, 0, 1, 2
        assert len({bytes(x) for x in dd[g][:, :8]}) == len(g)
    # tagff: both, ff alone, fe alone
    shapes = []
    for g in rc["tagff"]:
        tags = [dd[r][8:12].tobytes() for r in g]
        shapes.append(tuple(sorted(tags)))
        assert set(dc.tag_of(dd[g]).tolist()) == {0xFFFFFFFE}
        if len(g) == 2:
            assert np.array_equal(np.delete(dd[g[0]], range(8, 12)), np.delete(dd[g[1]], range(8, 12)))
    ff, fe = b"\xff" * 4, b"\xfe\xff\xff\xff"
    assert sorted(shapes) == sorted([(fe, ff), (ff,), (fe,)])
    # boundary: both sides of every step, and the two ends -- where a part has rows
    pref = (dd[rc["boundary"][0], 0].astype(int) << 8 | dd[rc["boundary"][0], 1]).tolist()
    want = sorted({0, 0xFFFF} | {x for b in nc.boundaries(W) for x in (b - 1, b)})
    assert sorted(pref) == [p for p in want if (p * W) >> 16 in populated]
    for b in nc.boundaries(W):
        assert ((b - 1) * W) >> 16 == ((b * W) >> 16) - 1
    if W in (3, 5, 7):
        import test_dict_hash
        assert nc.boundaries(W) == test_dict_hash.BOUNDARIES[W]
    assert ds[rc["wildcard"][0][0]] == 0 and ds[rc["sizerule"][0][0]] == nc.S1
    a, b = rc["duprow"][0]
    assert np.array_equal(dd[a], dd[b]) and a < b and db[a] != db[b]
    assert set(db[rc["unhit"][0]].tolist()) == set(nc.UNHIT_BLOBS)
    assert len(set(own[rc["plain"][0]].tolist())) == len(populated)  # spread over the owners
    assert int(db.max()) + 1 == n_blobs and len(set(db.tolist())) >= 8


def _check_layer(nd, case, dec, kind):
    W, cl = nd.W, case.classes
    dg, ln = case.digests, case.lengths
    k, ref = dec["kind"], dec["ref"].astype(np.int64)
    own = dc.owner_of(dg, W)
    if kind == "one":
        assert (own == W - 1).all()
    elif kind == "avoid":
        assert (own != 0).all() and len(set(own.tolist())) == W - 1
    dd, ds, db = nd.rows[0], nd.rows[1], nd.rows[2]
    first = _first_rows(dd)
    for c in np.flatnonzero(k == DICT):
        assert ref[c] == first[bytes(dg[c])] and ds[ref[c]] in (0, ln[c])
    for cls, gs in cl.items():
        if cls.startswith("m_"):  # misses: never DICT
            assert (k[gs[0]] != DICT).all(), cls
            assert all(bytes(dg[c]) not in first for c in gs[0]), cls
    for cls in ("q_part_tagchain", "q_part_wrap", "q_tagff", "q_boundary", "q_wildcard", "q_duprow"):
        if cls in cl:
            assert (k[cl[cls][0]] == DICT).all(), cls
    if case.n < 257:
        return
    full = kind == "mixed"
    populated = [o for o in range(W) if nd.pm[o]]
    if full:
        assert {"q_part_tagchain", "m_tagchain", "q_part_wrap", "m_wrap", "q_tagff", "m_tagff", "q_boundary",
                "m_boundary", "q_wildcard", "q_sizerule", "q_duprow", "q_plain", "m_plain", "intra"} <= set(cl)
        if len(populated) < W:
            assert "m_empty" in cl
            assert {int(o) for o in own[cl["m_empty"][0]]} == set(range(W)) - set(populated)
        # a hit on each chain row, and a miss that walks each chain, per populated part
        hit_rows = set(ref[cl["q_part_tagchain"][0]].tolist())
        assert hit_rows == {int(r) for g in nd.row_classes["part_tagchain"] for r in g[:nc.CHAIN]}
        assert set(ref[cl["q_part_wrap"][0]].tolist()) == {int(r) for g in nd.row_classes["part_wrap"] for r in g}
        assert sorted(own[cl["m_tagchain"][0]].tolist()) == populated
        assert sorted(own[cl["m_wrap"][0]].tolist()) == populated
        g = cl["q_sizerule"][0]
        assert tuple(ln[g]) == (nc.S2, nc.S2, nc.S1) and tuple(k[g]) == (NEW, INTRA, DICT) and ref[g[1]] == g[0]
        assert ln[cl["q_wildcard"][0][0]] == 12345
        a, b = nd.row_classes["duprow"][0]
        assert ref[cl["q_duprow"][0][0]] == a
        # boundary queries on both sides of every step
        pq = set((dg[cl["m_boundary"][0], 0].astype(int) << 8 | dg[cl["m_boundary"][0], 1]).tolist())
        assert pq == {0, 0xFFFF} | {x for b in nc.boundaries(W) for x in (b - 1, b)}
        assert len(set(own.tolist())) == W
        hit_blobs = set(db[ref[k == DICT]].tolist())
        assert not hit_blobs & set(nc.UNHIT_BLOBS) and nc.DUP_BLOB not in hit_blobs and len(hit_blobs) >= 6
        refused = [c for c in range(case.n) if bytes(dg[c]) in first and k[c] != DICT]
        assert refused
    for cls in ("m_tagchain", "m_wrap"):  # the misses share what makes the chain
        for c in cl.get(cls, [[]])[0]:
            o = int(own[c])
            rows = nd.row_classes["part_tagchain" if cls == "m_tagchain" else "part_wrap"]
            g = next(g for g in rows if own_of_row(nd, g[0]) == o)
            if cls == "m_tagchain":
                assert (dd[g][:, :12] == dg[c][:12]).all()
            else:
                assert dc.home_slot(dg[c][None], nd.cap[o] - 1)[0] == nd.cap[o] - 2


def own_of_row(nd, r):
    return int(nd.owners[r])


@pytest.mark.parametrize("W,variant,n,kind", LAYERS, ids=[f"W{W}-{v}-{k}{n}" for W, v, n, k in LAYERS])
def test_oracle_equals_model_and_layer_classes_hold(W, variant, n, kind, oracle):
    nd = nc.get_dict(W, variant)
    case = nc.get_layer(W, variant, n, kind)
    assert case.n == n and case.lengths.min() >= 1 and case.digests.any(axis=1).all()
    dd, ds, db, di, duoff, _ = case.dict
    exp, st = expect(case)
    got, own = oracle.dedup(case.digests, case.lengths, dd, ds, db, di, case.align, duoff)
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != exp[f])
        assert not len(bad), (f, bad[:8], got[f][bad[:8]], exp[f][bad[:8]])
    assert (NONE if own is None else own) == st["own_blob_index"]
    _check_layer(nd, case, exp, kind)


@pytest.mark.parametrize("W", WS)
def test_extend_case_holds(W):
    ex = nc.get_extend(W)
    rows = np.concatenate([s[0] for s in ex.segs])
    seg_of = np.repeat(np.arange(3), [len(s[0]) for s in ex.segs])
    own = dc.owner_of(rows, W)
    counts = [[int(((own == o) & (seg_of == s)).sum()) for o in range(W)] for s in range(3)]
    assert counts == [ex.pm0, ex.k1, ex.k2]
    if W >= 3:
        assert ex.pm0[-1] == 0  # a part that owns nothing until the first extend
    for o in range(W):
        rec_cap, cap = nc.fork_caps(ex.pm0[o], ex.k1[o])
        assert cap == ex.cap1[o]
        n2 = ex.pm0[o] + ex.k1[o] + ex.k2[o]
        assert n2 <= rec_cap and 2 * n2 + 16 <= cap  # in place (dict_grow_plan)
        segs_c = [s for s, _ in ex.chain[o]]
        assert {1, 2} <= set(segs_c) and len(segs_c) >= (4 if ex.pm0[o] == 0 else 7)
        d = np.stack([x for _, x in ex.chain[o]])
        assert (d[:, :12] == d[0, :12]).all() and (dc.owner_of(d, W) == o).all()
        assert len({bytes(x) for x in d}) == len(d)
        twin = [i for i, (s, _) in enumerate(ex.chain[o]) if s == 2][0]
        diff = d[twin] != d[twin - 1]
        assert diff[31] and diff.sum() == 1 and ex.chain[o][twin - 1][0] == 1
        w = np.stack([x for _, x in ex.wrap[o]])
        assert {1, 2} <= {s for s, _ in ex.wrap[o]}
        assert (dc.home_slot(w, cap - 1) == cap - 2).all() and (dc.owner_of(w, W) == o).all()
        assert len({bytes(x) for x in w[:, :8]}) == len(w) >= 4
    first = _first_rows(rows)
    assert len(ex.repeats) == 3 * W
    for d in ex.repeats:  # d2's repeats of d1's digests: seen first in segment 1, again in 2
        hits = [j for j in range(len(rows)) if bytes(rows[j]) == bytes(d)]
        assert [int(seg_of[j]) for j in hits] == [1, 2] and first[bytes(d)] == hits[0]
    assert len({bytes(x) for x in ex.q}) == len(ex.q)
    assert sum(bytes(x) not in first for x in ex.q) == ex.n_miss == 3 * W


def test_builder_is_deterministic():
    for W, v in ((3, "full"), (8, "one_empty")):
        a, b = nc.get_dict(W, v), nc.build_dict(W, v)
        c = nc.build_dict(W, v, seed=nc.SEED + 1)
        assert a is not b and not np.array_equal(a.rows[0], c.rows[0])
        for x, y in zip(a.rows, b.rows):
            assert np.array_equal(x, y)
        assert a.row_classes.keys() == b.row_classes.keys()
        for k in a.row_classes:
            assert all(np.array_equal(x, y) for x, y in zip(a.row_classes[k], b.row_classes[k]))
        la, lb = nc.get_layer(W, v, 257), nc.build_layer(b, 257)
        assert np.array_equal(la.digests, lb.digests) and np.array_equal(la.lengths, lb.lengths)
        for k in la.classes:
            assert all(np.array_equal(x, y) for x, y in zip(la.classes[k], lb.classes[k]))
    ea, eb = nc.get_extend(5), nc.build_extend(5)
    assert np.array_equal(ea.q, eb.q)
    for x, y in zip(ea.segs, eb.segs):
        assert all(np.array_equal(p, r) for p, r in zip(x, y))
