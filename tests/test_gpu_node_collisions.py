"""Crafted-digest collision matrix on the node dict paths: csrc/node.hip
(partition by owner, local table ids against global entry ids, per-part
in-place extends) and the exchange kernels of csrc/dedup.hip (dict_probe_owned,
hits_merge, route_count, route_scatter, dict_probe_routed, dict_probe_blocks,
hits_scatter).

Every other node test hashes real random bytes at W = 2, 4, 8, and with real
BLAKE3 output the places where this code can go wrong never run: an equal tag
on an unequal digest inside one part's table, a chain that wraps a part's small
table, the tag remap, a part that owns no row (a 16-slot table, dict.m == 0),
every query of a call going to one owner, a prefix exactly on an owner boundary
of a W that is no power of two, an older handle that must stay blind to rows
appended in place behind it on a part (e >= dict.m compares local ids), and the
grid-stride loop of dict_probe_routed (more than 2048 x 256 rows for one owner).

The cases of node_cases.py hold all of them.  Crafted records reach the
exchange through the product ABI: node.engines[i].set_dict(node_dict), then
ngpu_dedup_device without hits, which probes the node dict with the digests in
the records (marked NGPU_DIGESTED, no byte hashed).  Every field of every chunk
and every stats field must equal test_dedup_cases.model_dedup over the WHOLE
row list (equal to the oracle on every case: test_node_cases.py), and the
bytes a plain Engine gives under ngpu_dict_create of the same rows.

Real-hash entries (ngpu_node_process_device, ngpu_node_process_step, a
streaming Pack) run under SHA-256 over eight-byte chunks found by one hashlib
pass over 2^20 counters: real chunks on both sides of every owner boundary of
W = 3, real chunks all of one owner, each real digest between decoy rows that
copy its bytes 0-11.
"""
import hashlib
import io
import tarfile

import numpy as np
import pytest

import dedup_cases as dc
import node_cases as nc
import nydus_gpu
from nydus_gpu import rafs
from test_dedup_cases import DICT, NEW, NONE, expect, model_dedup
from test_gpu_dedup_collisions import STAT_FIELDS, _chunks, _compare, _dev, _records

pytestmark = pytest.mark.gpu

MODES = {"copy": nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_COPY,
         "routed": nydus_gpu.NODE_DICT_PARTITION | nydus_gpu.NODE_EXCHANGE_ROUTED,
         "replicate": nydus_gpu.NODE_DICT_REPLICATE}
WS = (2, 3, 5, 8)
MATRIX = [(W, m) for W in WS for m in MODES]
IDS = [f"W{W}-{m}" for W, m in MATRIX]
_EXPECT = {}   # case name -> (decisions, stats): the model, once per case
_PLAIN = {}    # case name -> (record bytes, stats) of the plain Engine: path against path


def _requesters(W):
    return list(range(W)) if W == 3 else [0, W - 1]


@pytest.fixture(scope="module")
def node_of():
    """One Node per (W, mode, digester), reused by every case that asks for it;
    the previous one is closed when another is asked for."""
    held = {}

    def get(W, mode, digester="blake3", chunk_size=dc.CHUNK_SIZE):
        key = (W, mode, digester, chunk_size)
        if key not in held:
            for n in held.values():
                n.close()
            held.clear()
            held[key] = nydus_gpu.Node([0] * W, digester=digester, chunk_size=chunk_size)
        return held[key]

    yield get
    for n in held.values():
        n.close()


@pytest.fixture(scope="module")
def plain():
    eng = nydus_gpu.Engine(chunk_size=dc.CHUNK_SIZE)
    yield eng
    eng.close()


def _recs80(rows):
    dd, ds, db, di, duoff = rows[:5]
    r = np.zeros(len(ds), rafs.CHUNK_INFO_DTYPE)
    r["block_id"], r["uncompressed_size"], r["blob_index"] = dd, ds, db
    r["index"], r["uncompressed_offset"] = di, duoff
    r["compressed_offset"] = np.arange(len(ds), dtype=np.uint64) * 4096 + 17
    r["compressed_size"] = 4000
    r["flags"] = 1
    return r


def _dedup(eng, case, shape=None):
    """One dedup call over fresh crafted records on engine `eng` (its default
    dict answers) -> (records, list of layer stats)."""
    import torch
    d_ch, out = _dev(_chunks(case)), _dev(_records(case))
    if shape is None:
        stats = [eng.dedup_device(d_ch.data_ptr(), case.n, out.data_ptr(), want_stats=True)]
    else:
        L = len(shape) - 1
        d_first = torch.from_numpy(np.asarray(shape, np.int64)).cuda()
        d_st = torch.zeros(L * nydus_gpu.LAYER_STATS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        eng.dedup_layers_device(d_ch.data_ptr(), case.n, out.data_ptr(), d_first.data_ptr(), L, d_st.data_ptr())
        torch.cuda.synchronize()
        stats = list(d_st.cpu().numpy().view(nydus_gpu.LAYER_STATS_DTYPE))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
    eng.device_status()
    return got, stats


def _stat_tuple(stats):
    return [tuple(int(s[f]) for f in STAT_FIELDS) for s in stats]


def _layers_expect(case, first):
    """Each layer's slice alone under the whole dict; NEW / INTRA refs are
    chunk ids of the call."""
    dd, ds, db, di, duoff, _ = case.dict
    dec, stats = [], []
    for a, b in zip(first[:-1], first[1:]):
        e, st = model_dedup(case.digests[a:b], case.lengths[a:b], dd, ds, db, di, duoff, case.align)
        e["ref"][e["kind"] != DICT] += a
        dec.append(e)
        stats.append(st)
    return np.concatenate(dec), stats


def _run_case(node, d, plain, plain_dict, case, W, mode, shape=None):
    key = case.name + ("" if shape is None else f"-L{list(shape)}")
    if key not in _EXPECT:
        if shape is None:
            exp, st = expect(case)
            _EXPECT[key] = (exp, [st])
        else:
            _EXPECT[key] = _layers_expect(case, shape)
    exp, est = _EXPECT[key]
    if key not in _PLAIN:
        plain.set_dict(plain_dict)
        got, stats = _dedup(plain, case, shape)
        _compare(f"plain engine {key}", case, got, stats, exp, est)
        _PLAIN[key] = (got.tobytes(), _stat_tuple(stats))
    for i in _requesters(W):
        node.engines[i].set_dict(d)
        got, stats = _dedup(node.engines[i], case, shape)
        tag = f"W{W} {mode} requester {i} {key}"
        _compare(tag, case, got, stats, exp, est)
        assert (got.tobytes(), _stat_tuple(stats)) == _PLAIN[key], f"{tag}: differs from the plain engine"


def _release(node, *dicts):
    for e in node.engines:
        e.set_dict(None)
    for d in dicts:
        d.release()


@pytest.mark.parametrize("W,mode", MATRIX, ids=IDS)
def test_node_collision_matrix(W, mode, node_of, plain):
    """The node_cases cases at n = 1, 64, 257 and 4097 through
    ngpu_dedup_device on the node's engines: every variant's mixed layer, the
    full dict's one-owner and avoid-one-owner layers, and one case through
    ngpu_dedup_layers_device with an empty middle layer."""
    node = node_of(W, mode)
    for variant in nc.VARIANTS:
        nd = nc.get_dict(W, variant)
        recs = _recs80(nd.rows)
        d = node.dict_create(recs, mode=MODES[mode])
        pd = plain.dict_create(recs)
        try:
            assert d.entries == nd.m and d.info()["blobs"] == nc.N_BLOBS
            for n in nc.LAYER_N:
                _run_case(node, d, plain, pd, nc.get_layer(W, variant, n), W, mode)
            if variant == "full":
                for kind in ("one", "avoid"):
                    for n in (257, 4097):
                        _run_case(node, d, plain, pd, nc.get_layer(W, variant, n, kind), W, mode)
                _run_case(node, d, plain, pd, nc.get_layer(W, variant, 257), W, mode, shape=[0, 85, 85, 257])
        finally:
            plain.set_dict(None)
            _release(node, d, pd)


@pytest.mark.parametrize("W,mode", MATRIX, ids=IDS)
def test_dedup_cases_under_a_node_dict(W, mode, node_of, plain):
    """The mixed-with-dict cases of dedup_cases.py at 257 and 4097 chunks: rows
    built for one table, spread over W small ones; the few rows of the 257
    case leave most parts of W = 5 and 8 with 0-5 rows."""
    node = node_of(W, mode)
    for n in (257, 4097):
        case = dc.get("mixed", n, 4096, True)
        recs = _recs80(case.dict)
        if n == 257 and W >= 5:
            assert (np.bincount(dc.owner_of(case.dict[0], W), minlength=W) <= 5).sum() > W // 2
        d = node.dict_create(recs, mode=MODES[mode])
        pd = plain.dict_create(recs)
        try:
            _run_case(node, d, plain, pd, case, W, mode)
        finally:
            plain.set_dict(None)
            _release(node, d, pd)


# ---- the grid stride of dict_probe_routed -------------------------------------------
def test_routed_probe_grid_stride(node_of, oracle):
    """2048 x 256 + 300 distinct crafted digests, all of owner 1 of 2: the
    routed probe's grid (at most 2048 workgroups of 256) strides.  About 2,000
    dict rows, 320 of them hit, the last 300 chunks among them.  Expected: the
    C oracle; the copy exchange must give the same bytes."""
    import torch
    n, W = 2048 * 256 + 300, 2
    rng = np.random.default_rng(20241021)
    dg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    dg[:, 16:24] = (np.arange(n, dtype="<u8") + 1).view(np.uint8).reshape(n, 8)
    dg[:, 0] |= 0x80
    assert (dc.owner_of(dg, W) == 1).all()
    lengths = np.full(n, dc.CHUNK_SIZE, np.uint32)
    hit = np.concatenate([np.arange(7, n - 300, (n - 300) // 20)[:20], np.arange(n - 300, n)])
    other = rng.integers(0, 256, (1700, 32), dtype=np.uint8)
    other[:, 16:24] = (np.arange(1700, dtype="<u8") + (1 << 40)).view(np.uint8).reshape(1700, 8)
    dd = np.concatenate([other[:900], dg[hit], other[900:]])
    order = rng.permutation(len(dd))
    dd = dd[order]
    m = len(dd)
    ds = np.where(np.arange(m) % 3 == 0, 0, dc.CHUNK_SIZE).astype(np.uint32)
    db = (np.arange(m) % 5).astype(np.uint32)
    di = (np.arange(m) * 3 + 11).astype(np.uint32)
    duoff = (np.arange(m, dtype=np.uint64) + 1) * np.uint64(0x1000)
    exp, own = oracle.dedup(dg, lengths, dd, ds, db, di, 4096, duoff)
    assert (exp["kind"] == DICT).sum() == len(hit) and (exp["kind"][-300:] == DICT).all()
    assert (exp["kind"][exp["kind"] != DICT] == NEW).all()
    new = exp["kind"] == NEW
    est = {"chunks": n, "new_chunks": int(new.sum()), "intra_chunks": 0, "dict_chunks": len(hit),
           "new_bytes": int(new.sum()) * dc.CHUNK_SIZE, "own_blob_index": NONE if own is None else own,
           "blobs": len(set(db[exp["ref"][~new].astype(np.int64)].tolist())) + 1,
           "uncompressed_size": int(new.sum()) * dc.CHUNK_SIZE}
    case = dc.Case("stride", dg, lengths, (dd, ds, db, di, duoff, 5), {}, 4096)
    recs = _recs80(case.dict)
    rec0 = _records(case)
    ch = np.zeros(n, nydus_gpu.CHUNK_DTYPE)
    ch["length"] = lengths
    d_ch = _dev(ch)
    seen = {}
    for mode in ("routed", "copy"):
        node = node_of(W, mode)
        d = node.dict_create(recs, mode=MODES[mode])
        try:
            node.engines[0].set_dict(d)
            out = _dev(rec0)
            st = node.engines[0].dedup_device(d_ch.data_ptr(), n, out.data_ptr(), want_stats=True)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
            del out
            node.engines[0].device_status()
            _compare(f"stride {mode}", case, got, [st], exp, [est])
            seen[mode] = hashlib.sha256(got.tobytes()).digest()
        finally:
            _release(node, d)
    assert seen["routed"] == seen["copy"]


# ---- blindness per part ---------------------------------------------------------------
def _concat_rows(segs, upto):
    """The rows create(segs[0]) + extends stand for: each extension's blob
    indices count from the blob count before it (max index + 1, no tables)."""
    cols, shift = [[] for _ in range(5)], 0
    for dd, ds, db, di, duoff in segs[:upto]:
        for c, x in zip(cols, (dd, ds, db + np.uint32(shift), di, duoff)):
            c.append(x)
        shift += int(db.max()) + 1
    return tuple(np.concatenate(c) for c in cols) + (shift,)


@pytest.mark.parametrize("W,mode", MATRIX, ids=IDS)
def test_older_handles_stay_blind_per_part(W, mode, node_of, plain):
    """d0 = create, d1 = extend (every part forks), d2 = extend (every part in
    place).  The appended rows continue d1's tag chain and wrapping chain on
    every part and repeat d1's digests.  With d2 alive, d1 answers for exactly
    its own rows and d0 for its own; each equals a plain Engine's dict of the
    handle's rows."""
    node = node_of(W, mode)
    ex = nc.get_extend(W)
    recs = [_recs80(s) for s in ex.segs]
    d0 = node.dict_create(recs[0], mode=MODES[mode])
    d1 = node.dict_extend(d0, recs[1])
    d2 = node.dict_extend(d1, recs[2])
    pds = []
    try:
        lens = np.cumsum([len(r) for r in recs]).tolist()
        assert [d0.entries, d1.entries, d2.entries] == lens
        i0, i1, i2 = d0.info(), d1.info(), d2.info()
        assert not i0["shares_base_storage"] and not i1["shares_base_storage"] and i2["shares_base_storage"]
        # info() reports part 0 (replicate: a replica, which holds every row)
        m0, k1 = (lens[0], lens[1] - lens[0]) if mode == "replicate" else (ex.pm0[0], ex.k1[0])
        caps = nc.fork_caps(m0, k1)
        assert (i0["record_capacity"], i0["table_capacity"]) == (m0, nc.part_cap(m0))
        assert (i1["record_capacity"], i1["table_capacity"]) == caps
        assert (i2["record_capacity"], i2["table_capacity"]) == caps
        assert [x["blobs"] for x in (i0, i1, i2)] == [3, 6, 9]
        lengths = np.full(len(ex.q), dc.CHUNK_SIZE, np.uint32)
        hits = []
        for label, d, upto in (("d2", d2, 3), ("d1", d1, 2), ("d0", d0, 1), ("d1 again", d1, 2)):
            rows = _concat_rows(ex.segs, upto)
            case = dc.Case(f"extend-W{W}-{upto}", ex.q, lengths, rows, {}, 4096)
            pd = plain.dict_create(_recs80(rows))
            pds.append(pd)
            _run_case(node, d, plain, pd, case, W, f"{mode} {label}")
            exp = _EXPECT[case.name][0]
            hits.append(int((exp["kind"] == DICT).sum()))
            seen = {bytes(x) for x in rows[0]}
            assert hits[-1] == sum(bytes(x) in seen for x in ex.q)
        assert hits[0] > hits[1] > hits[2] > 0 and hits[3] == hits[1]
    finally:
        plain.set_dict(None)
        _release(node, d2, d1, d0, *pds)


# ---- real hashes: SHA-256 over eight-byte chunks ---------------------------------------
@pytest.fixture(scope="module")
def counters():
    """SHA-256 of the 2^20 eight-byte little-endian counters -> (digests,
    counters by 16-bit prefix)."""
    n = 1 << 20
    raw = (np.arange(n, dtype="<u8")).tobytes()
    sha = hashlib.sha256
    dig = np.frombuffer(b"".join(sha(raw[8 * i:8 * i + 8]).digest() for i in range(n)), np.uint8).reshape(n, 32)
    prefix = dig[:, 0].astype(np.int64) << 8 | dig[:, 1]
    order = np.argsort(prefix, kind="stable")
    starts = np.searchsorted(prefix[order], np.arange(65537))
    return dig, order, starts


def _with_prefix(counters, p, k=1):
    _, order, starts = counters
    got = order[starts[p]:starts[p + 1]][:k]
    assert len(got) == k, f"no counter with prefix {p:#x}"
    return [int(x) for x in got]


def _of_owner(counters, W, o, k, skip=0):
    lo, _ = nc.prefix_range(W, o)
    _, order, starts = counters
    return [int(x) for x in order[starts[lo] + skip:starts[lo] + skip + k]]


def _real_layer(ids):
    """Chunks of 8 bytes, back to back: (data, chunk descriptors)."""
    data = np.asarray(ids, dtype="<u8").view(np.uint8)
    ch = np.zeros(len(ids), nydus_gpu.CHUNK_DTYPE)
    ch["offset"] = np.arange(len(ids)) * 8
    ch["length"] = 8
    ch["file_index"] = np.arange(len(ids))
    return np.concatenate([data, np.zeros(64, np.uint8)]), ch


def _decoy_dict(counters, ids, rng):
    """Every real digest of `ids` between two decoy rows that copy its bytes
    0-11 (same owner, home slot and tag, another tail)."""
    dig = counters[0]
    rows = []
    for i in ids:
        for k in range(3):
            d = dig[i].copy()
            if k != 1:
                d[12:] = rng.integers(0, 256, 20, dtype=np.uint8)
            rows.append(d)
    dd = np.stack(rows)
    m = len(dd)
    return (dd, np.where(np.arange(m) % 2, 8, 0).astype(np.uint32), (np.arange(m) % 4).astype(np.uint32),
            (np.arange(m) + 100).astype(np.uint32), (np.arange(m, dtype=np.uint64) + 1) * np.uint64(4096))


def _expect_real(oracle, counters, ids, rows):
    dig = counters[0][np.asarray(ids, np.int64)] if len(ids) else np.zeros((0, 32), np.uint8)
    dd, ds, db, di, duoff = rows
    dec, _ = oracle.dedup(dig, np.full(len(ids), 8, np.uint32), dd, ds, db, di, 4096, duoff)
    return dig, dec


def _same(tag, got, dig, dec):
    assert np.array_equal(got["digest"], dig), f"{tag}: digest differs from hashlib"
    for f in ("kind", "index", "ref", "blob_index", "uncompressed_offset"):
        assert np.array_equal(got[f], dec[f]), (tag, f)


REAL = [(W, m) for W in (3, 8) for m in MODES]


@pytest.mark.parametrize("W,mode", REAL, ids=[f"W{W}-{m}" for W, m in REAL])
def test_real_sha256_chunks_through_the_node_entries(W, mode, node_of, oracle, counters):
    """ngpu_node_process_device on every requester, two ngpu_node_process_step
    calls in a row (parts of n = 0, n = 1, all to one owner, none to one owner,
    mixed) and one streaming Pack, on real SHA-256 digests at the owner
    boundaries; hashlib is the digest reference, oracle.dedup with the whole
    dict the decision reference, per layer."""
    import torch
    rng = np.random.default_rng(500 + W)
    cs = 0x10000
    edge = [c for p in sorted({0, 0xFFFF} | {x for b in nc.boundaries(W) for x in (b - 1, b)})
            for c in _with_prefix(counters, p, 2)]
    assert sorted(set(dc.owner_of(counters[0][edge], W).tolist())) == list(range(W))
    per_owner = [_of_owner(counters, W, o, 40, skip=5) for o in range(W)]
    known = edge[::2] + [c for po in per_owner for c in po[:20]]      # in the dict
    rows = _decoy_dict(counters, known, rng)
    recs = _recs80(rows)

    def mixed(k):
        pool = edge + [c for po in per_owner for c in po[10:30] + po[22:26]]  # (repeats: INTRA)
        return [int(x) for x in rng.permutation(pool)][:k]

    one = per_owner[1][5:35] + per_owner[1][16:24]                     # all to owner 1, some repeated
    avoid = [c for o, po in enumerate(per_owner) if o != 0 for c in po[15:25]]
    kinds = [[], [edge[0]], one, avoid] + [mixed(60 + 7 * j) for j in range(max(W - 4, 1))]
    node = node_of(W, mode, "sha256", cs)
    d = node.dict_create(recs, mode=MODES[mode])
    keep = []
    try:
        def part(ids):
            data, ch = _real_layer(ids)
            t = (_dev(data), _dev(ch) if len(ids) else None,
                 torch.zeros(max(len(ids), 1) * 64, dtype=torch.uint8, device="cuda"))
            keep.append(t)
            return t

        # one layer per requester through ngpu_node_process_device
        for i in range(W):
            ids = mixed(50 + i) if i else edge
            buf, dch, out = part(ids)
            node.process_device(i, d, buf.data_ptr(), buf.numel(), dch.data_ptr(), len(ids), out.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            dig, dec = _expect_real(oracle, counters, ids, rows)
            _same(f"process_device {i}", out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)[:len(ids)], dig, dec)
            assert (dec["kind"] == DICT).any() and (dec["kind"] != DICT).any()
        # two steps in a row; between them the part kinds move on by three
        assert len(kinds) >= 5 and (W == 3 or len(kinds) == W)
        for step in range(2):
            layout = [kinds[(i + 3 * step) % len(kinds)] for i in range(W)]
            parts, outs = [], []
            for ids in layout:
                buf, dch, out = part(ids)
                outs.append(out)
                parts.append({"d_data": buf.data_ptr(), "len": buf.numel(),
                              "d_chunks": dch.data_ptr() if dch is not None else 0, "n": len(ids),
                              "d_out": out.data_ptr()})
            torch.cuda.synchronize()
            node.process_step(d, parts)
            torch.cuda.synchronize()
            for i, (ids, out) in enumerate(zip(layout, outs)):
                dig, dec = _expect_real(oracle, counters, ids, rows)
                _same(f"step {step} part {i}", out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)[:len(ids)], dig, dec)
        for e in node.engines:
            e.device_status()
        # one streaming Pack: a tar of eight-byte files
        ids = mixed(48)
        tar = io.BytesIO()
        with tarfile.open(fileobj=tar, mode="w", format=tarfile.USTAR_FORMAT) as tf:
            for c in ids:
                ti = tarfile.TarInfo(f"f{c:08d}")
                ti.size = 8
                tf.addfile(ti, io.BytesIO(int(c).to_bytes(8, "little")))
        tar = tar.getvalue()
        w = node.pack(d)
        w.write(tar)
        ch, out, st = w.close()
        ech = oracle.tar_chunks(tar, cs)
        assert ch.tobytes() == ech.tobytes() and len(ch) == len(ids)
        dig = np.stack([np.frombuffer(hashlib.sha256(tar[int(c["offset"]):int(c["offset"]) + int(c["length"])]).digest(),
                                      np.uint8) for c in ech])
        assert sorted(bytes(x) for x in dig) == sorted(bytes(counters[0][c]) for c in ids)
        dec, _ = oracle.dedup(dig, ech["length"], *rows[:4], 4096, rows[4])
        _same("pack", out, dig, dec)
        assert st["dict_chunks"] == int((dec["kind"] == DICT).sum()) > 0
    finally:
        _release(node, d)
