"""Dict distill (ngpu_dict_distill, include/nydus_gpu.h): the sequential model
and the crafted dicts the tests share.  A helper, not a test.

The model is the header's definition read aloud over 80-B records and 256-B blob
rows: the first row of every digest, how many rows hold it, the min_refs filter,
the blob rule per flag, and the info fields.  The hash rules (home slot, tag) are
dedup_cases.py's, not restated here."""
import numpy as np

import dedup_cases as dc
from nydus_gpu import rafs

KEEP_BLOBS, MERGE_BLOB_IDS = 0x1, 0x2
INFO_FIELDS = ("entries_in", "distinct", "shadowed", "below_min", "entries_out", "blobs_in", "blobs_out",
               "max_refs", "refs_hist")
assert dc.GOLDEN == 0x9E3779B97F4A7C15


def pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def caps(s):
    """dict_retire_plan.hpp: record and table capacity of a result of s survivors."""
    cap = s + s // 2
    return cap, pow2(2 * cap + 16)


def created_table_cap(m):
    """The table ngpu_dict_create gives a dict of m rows."""
    return pow2(2 * m + 16)


def rows(rng, m, blobs, usize=0x10000):
    """m random 80-B records (every field a dict keeps set) in the given blobs."""
    r = np.zeros(m, rafs.CHUNK_INFO_DTYPE)
    r["block_id"] = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    r["blob_index"] = blobs
    r["uncompressed_size"] = usize
    r["index"] = rng.integers(0, 1 << 20, m)
    r["uncompressed_offset"] = rng.integers(0, 1 << 30, m).astype(np.uint64) * 4096
    r["compressed_offset"] = rng.integers(0, 1 << 40, m)
    r["compressed_size"] = rng.integers(1, 1 << 16, m)
    r["flags"] = rng.integers(0, 2, m)
    return r


def table(ids, cs=0x10000):
    """256-B blob rows for the given ids (ints or 64-hex strings) -> (n, 256) u8."""
    ids = [f"{i:064x}" if isinstance(i, int) else i for i in ids]
    return np.ascontiguousarray(rafs.make_blob_table(ids, cs)).view(np.uint8).reshape(-1, 256)


def refs_of(recs):
    """-> (winner row of every row, refs of every row's digest), sequentially."""
    first, count = {}, {}
    win = np.zeros(len(recs), np.int64)
    for i, d in enumerate(recs["block_id"]):
        k = d.tobytes()
        win[i] = first.setdefault(k, i)
        count[win[i]] = count.get(win[i], 0) + 1
    return win, np.array([count[w] for w in win], np.int64)


def model(recs, nb, tbl=None, min_refs=1, flags=0):
    """-> (surviving records, their blob rows as bytes or None, info dict).
    recs: the base's rows in table order; nb: its blob count; tbl: its (nb, 256)
    blob rows or None."""
    m = len(recs)
    win, refs = refs_of(recs)
    is_win = win == np.arange(m)
    need = max(int(min_refs), 1)
    keep = is_win & (refs >= need)
    out = recs[keep].copy()
    live = np.zeros(nb, bool)
    inside = out["blob_index"] < nb
    live[out["blob_index"][inside]] = True
    if flags & KEEP_BLOBS:
        remap, kept = np.arange(nb, dtype=np.uint32), list(range(nb))
    else:
        rep = list(range(nb))
        if flags & MERGE_BLOB_IDS and tbl is not None:
            seen = {}
            rep = [seen.setdefault(tbl[b, :64].tobytes(), b) for b in range(nb)]
        alive = np.zeros(nb, bool)
        for b in range(nb):
            alive[rep[b]] |= live[b]
        kept = [b for b in range(nb) if rep[b] == b and alive[b]]
        rank = {b: i for i, b in enumerate(kept)}
        remap = np.array([rank.get(rep[b], 0xFFFFFFFF) for b in range(nb)], np.uint32)
    if inside.any():
        out["blob_index"][inside] = remap[out["blob_index"][inside]]
        assert (out["blob_index"][inside] != 0xFFFFFFFF).all()
    hist = [0] * 32
    for r in refs[is_win]:
        hist[int(r).bit_length() - 1] += 1
    distinct = int(is_win.sum())
    info = {"entries_in": m, "distinct": distinct, "shadowed": m - distinct,
            "below_min": int((is_win & (refs < need)).sum()), "entries_out": len(out), "blobs_in": nb,
            "blobs_out": len(kept), "max_refs": int(refs.max()) if m else 0, "refs_hist": hist}
    out_tbl = None if tbl is None or not len(kept) else np.ascontiguousarray(tbl[kept]).tobytes()
    return out, out_tbl, info


def expect_hits(recs, q, hit_dtype, miss):
    """Plain first-occurrence scan of the 80-B rows for every query digest."""
    first = {}
    for j, d in enumerate(recs["block_id"]):
        first.setdefault(d.tobytes(), j)
    exp = np.zeros(len(q), hit_dtype)
    for i in range(len(q)):
        j = first.get(q[i].tobytes())
        if j is None:
            exp[i]["entry"] = miss
        else:
            r = recs[j]
            exp[i] = (j, r["index"], r["blob_index"], r["uncompressed_size"], r["uncompressed_offset"])
    return exp


# ---- row patterns ------------------------------------------------------------------------
def pattern(name, rng, m, nb=3):
    """m rows of the named duplicate pattern, in blobs [0, nb)."""
    r = rows(rng, m, rng.integers(0, nb, m) if m else 0)
    dd = r["block_id"]
    if name == "distinct" or m == 0:
        pass
    elif name == "one":                       # one digest in every row
        dd[:] = dd[0]
    elif name.startswith("dist"):             # a duplicate at that distance from its winner
        k = int(name[4:])
        if 0 < k < m:
            dd[k] = dd[0]
            for a in range(1, m - k, max(1, m // 7)):  # and a few more pairs of the same distance
                if (dd[a] != dd[0]).any() and (dd[a + k] != dd[0]).any():
                    dd[a + k] = dd[a]
    elif name == "last":                      # distance m - 1
        dd[m - 1] = dd[0]
    elif name == "triples":
        for a in range(0, m - 2, 3):
            dd[a + 1] = dd[a + 2] = dd[a]
        if m >= 9:                            # and triples spread over the dict
            dd[m // 2] = dd[m - 1] = dd[1 + 3 * (m // 9)]
    elif name == "keys":
        # whole waves of rows that all lose: wave w >= 1 repeats 1, 2, 8, 9, 20, 64
        # digests of wave 0 (the in-wave aggregation takes 8 keys, then lanes go alone)
        for w, k in enumerate((1, 2, 8, 9, 20, 64), start=1):
            for j in range(64):
                if 64 * w + j < m:
                    dd[64 * w + j] = dd[(j * 7) % k]
    elif name == "usize":                     # equal digests with unequal usize: one digest
        for a in range(0, m - 1, 2):
            dd[a + 1] = dd[a]
            r["uncompressed_size"][a + 1] = r["uncompressed_size"][a] - 1 - (a % 7)
        r["uncompressed_size"][::5] = 0
    else:
        raise ValueError(name)
    return r


PATTERNS = ("distinct", "one", "dist1", "dist63", "dist64", "dist65", "dist256", "last", "triples", "keys",
            "usize")


# ---- crafted digests -----------------------------------------------------------------------
def words_homed(rng, slot, mask, count):
    found = []
    while len(found) < count:
        w = rng.integers(0, np.iinfo(np.uint64).max, 1 << 18, dtype=np.uint64, endpoint=True)
        found.extend(int(x) for x in w[dc.home_slot(w.view(np.uint8).reshape(-1, 8), mask) == np.uint64(slot)])
    return list(dict.fromkeys(found))[:count]


def crafted(rng, m=4096):
    """m rows over a created dict's table: 14 rows share bucket words and tag on
    unequal digests (one chain walked by digest compares), 7 are homed two slots
    before the end of the table (the chain wraps), 6 share bucket words with word 2
    0xFFFFFFFF / 0xFFFFFFFE (one stored tag), and every group has duplicates:
    some before, some after other members of their chain.  -> (rows, the special
    rows' indices)."""
    cap = created_table_cap(m)
    r = rows(rng, m, rng.integers(0, 4, m))
    dd = r["block_id"]
    coll = [100, 200, 300, 400, 500, 600, 700, 800, 1000, 1100, 1200, 1300, 3100, 3200]
    for x in coll:
        dd[x, :12] = dd[100, :12]
    wrap = [10, 20, 660, 670, 3010, 3020, 3030]
    for x, w in zip(wrap, words_homed(rng, cap - 2, cap - 1, len(wrap))):
        dd[x, :8] = np.frombuffer(np.uint64(w).tobytes(), np.uint8)
    tags = [40, 41, 1500, 1501, 3900, 3901]
    for j, x in enumerate(tags):
        dd[x, :8] = dd[40, :8]
        dd[x, 8:12] = (0xFF, 0xFF, 0xFF, 0xFF) if j % 2 == 0 else (0xFE, 0xFF, 0xFF, 0xFF)
    assert len(set(dc.tag_of(dd[tags]))) == 1 and len(set(dc.tag_of(dd[coll]))) == 1
    assert len(set(int(x) for x in dc.home_slot(dd[coll], cap - 1))) == 1
    assert set(int(x) for x in dc.home_slot(dd[wrap], cap - 1)) == {cap - 2}
    dups = {900: 300, 901: 300, 750: 700, 3500: 3010, 3501: 20, 3950: 1500, 3951: 1501, 3300: 3200,
            4000: 100, 4001: 100, 4002: 100}
    for a, b in dups.items():
        dd[a] = dd[b]
    return r, coll + wrap + tags + list(dups)
