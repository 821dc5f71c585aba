"""Crafted digests for the node dict paths (test_node_cases.py on the CPU,
test_gpu_node_collisions.py on the GPU): csrc/node.hip and the exchange
kernels of csrc/dedup.hip.

In the style of dedup_cases.py: numpy only, every generator seeded, nothing
imported from the GPU library.  A W-part node dict keeps the rows whose digest
prefix maps to owner o (dedup_cases.owner_of) on part o, in a table of its own
of pow2(2 pm + 16) slots (pm: the part's row count), with local table ids and
global entry ids.  A dict here is the whole row list in table order (80-byte
records are made of it by the GPU test); the expectation is
test_dedup_cases.model_dedup over that whole list, whatever W is.

Row classes (NodeDict.row_classes: name -> groups of row numbers):
  part_tagchain  per populated part: 6 rows sharing bytes 0-11 (one owner, home
                 slot and tag); row 1 is row 0 with byte 31 changed; two later
                 rows repeat rows 0 and 2 in another blob (never the answer):
                 a group is [the 6, then the 2 repeats]
  part_wrap      per populated part: 5 rows with different bucket words homed at
                 the part's cap - 2, so the chain wraps to slot 0
  tagff          pairs with tag words 0xFFFFFFFF / 0xFFFFFFFE, otherwise equal:
                 both as rows; only the ff one; only the fe one
  boundary       a row at prefix b - 1 and one at b for every owner boundary b
                 (the prefix steps there: ceil(k 65536 / W)), and at 0x0000 and
                 0xFFFF -- where the part is populated
  wildcard       a row of usize 0 (hit at an odd length)
  sizerule       a row of usize S1 met by chunks of (S2, S2, S1): NEW, INTRA, DICT
  duprow         a digest on two rows in different blobs
  unhit          rows in blobs no chunk hits
  plain          well-distributed rows of random owners
Variants: "full" (every part populated), "one_empty" (part W // 2 owns no row),
"one_owner" (part W - 1 owns every row).

Layer classes (Case.classes, chunk ids): q_<row class> for hits, and
  m_tagchain     per part, bytes 0-11 of the chain and a fresh tail: walks it all
  m_wrap         per part, the bucket words of a wrap row and a fresh tag / tail
  m_tagff        the absent twin of the one-sided tagff pairs
  m_boundary     a fresh digest at every boundary prefix (both sides)
  m_empty        fresh digests owned by the parts without rows
  m_plain, intra fresh misses, and repeats of earlier chunks
Layer kinds: "mixed"; "one" (every chunk belongs to owner W - 1); "avoid" (no
chunk belongs to owner 0).
"""
import numpy as np

import dedup_cases as dc

CHUNK_SIZE, S1, S2 = dc.CHUNK_SIZE, dc.S1, dc.S2
N_BLOBS = 9                  # rows name blobs 0..8; 3 and 6 are never hit
UNHIT_BLOBS = (3, 6)
DUP_BLOB = 8                 # the later rows of a repeated digest
SEED = 20241020
VARIANTS = ("full", "one_empty", "one_owner")
KINDS = ("mixed", "one", "avoid")
LAYER_N = (1, 64, 257, 4097)
CHAIN, WRAP = 6, 5


def pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


def part_cap(pm):
    """Table capacity of a part of pm rows (dict_table_cap)."""
    return pow2(2 * pm + 16)


def boundaries(W):
    """The prefixes at which the owner steps: ceil(k 65536 / W), k = 1..W-1."""
    return [-(-k * 65536 // W) for k in range(1, W)]


def prefix_range(W, o):
    return -(-o * 65536 // W), -(-(o + 1) * 65536 // W) - 1


class NodeDict:
    """rows = (dd, ds, db, di, duoff, n_blobs) in table order; row_classes;
    pm / cap: rows and table slots per part."""

    def __init__(self, name, W, variant, rows, row_classes, queries):
        self.name, self.W, self.variant = name, W, variant
        self.rows, self.row_classes, self.queries = rows, row_classes, queries
        own = dc.owner_of(rows[0], W)
        self.owners = own
        self.pm = [int((own == o).sum()) for o in range(W)]
        self.cap = [part_cap(m) for m in self.pm]

    @property
    def m(self):
        return len(self.rows[1])


class _Gen:
    def __init__(self, W, seed, salt):
        self.W = W
        self.rng = np.random.default_rng([seed, W, salt])
        self.ctr = 0

    def prefix_in(self, o):
        lo, hi = prefix_range(self.W, o)
        return int(self.rng.integers(lo, hi + 1))

    def fresh(self, owner=None, prefix=None, words=None, tag=None, head12=None):
        d = self.rng.integers(0, 256, 32, dtype=np.uint8)
        self.ctr += 1
        d[16:24] = np.frombuffer(np.uint64(self.ctr).tobytes(), np.uint8)
        if owner is not None:
            prefix = self.prefix_in(owner)
        if prefix is not None:
            d[0], d[1] = prefix >> 8, prefix & 0xFF
        if words is not None:
            d[0:8] = np.frombuffer(np.uint64(words).tobytes(), np.uint8)
        if tag is not None:
            d[8:12] = np.frombuffer(np.uint32(tag).tobytes(), np.uint8)
        if head12 is not None:
            d[0:12] = head12
        return d

    def words_homed(self, owner, slot, mask, count):
        """`count` distinct bucket words of `owner` whose home slot (home_slot)
        in a table of mask + 1 slots is `slot`."""
        lo, hi = prefix_range(self.W, owner)
        found = []
        while len(found) < count:
            d = self.rng.integers(0, 256, (1 << 16, 8), dtype=np.uint8)
            p = self.rng.integers(lo, hi + 1, 1 << 16)
            d[:, 0], d[:, 1] = p >> 8, p & 0xFF
            hit = d[dc.home_slot(d, mask) == np.uint64(slot)]
            found.extend(int(x) for x in np.ascontiguousarray(hit).view("<u8")[:, 0])
            found = list(dict.fromkeys(found))
        return found[:count]


def _hit_blob(j):
    return (0, 1, 2, 4, 5, 7)[j % 6]


def build_dict(W, variant="full", seed=SEED):
    g = _Gen(W, seed, 1 + VARIANTS.index(variant))
    if variant == "full":
        populated = list(range(W))
    elif variant == "one_empty":
        populated = [o for o in range(W) if o != W // 2]
    else:
        populated = [W - 1]
    rows, classes = [], {}     # rows: [digest, usize, blob, class, after (row that must precede)]
    queries = []               # (class, digest, length, order key or None)

    def row(cls, d, usize, blob, after=None, new_group=True):
        r = len(rows)
        rows.append([d, usize, blob, cls, after])
        grp = classes.setdefault(cls, [])
        if new_group or not grp:
            grp.append([])
        grp[-1].append(r)
        return r

    def q(cls, d, length=CHUNK_SIZE, order=None):
        queries.append((cls, d, length, order))

    def any_owner():
        return populated[int(g.rng.integers(0, len(populated)))]

    # per part: the tag-collision chain
    for o in populated:
        head = g.fresh(owner=o, tag=int(g.rng.integers(0, 0xFFFFFFF0)))[:12].copy()
        mem = [g.fresh(head12=head) for _ in range(CHAIN)]
        mem[1] = mem[0].copy()
        mem[1][31] ^= 0x01
        ids = [row("part_tagchain", d, CHUNK_SIZE if j % 2 else 0, _hit_blob(j + o), new_group=(j == 0))
               for j, d in enumerate(mem)]
        for j in (0, 2):
            row("part_tagchain", mem[j], CHUNK_SIZE, DUP_BLOB, after=ids[j], new_group=False)
        for d in mem:
            q("q_part_tagchain", d)
        q("m_tagchain", g.fresh(head12=head))
    # tagff: both rows; ff alone; fe alone
    for k, (ff_row, fe_row) in enumerate(((True, True), (True, False), (False, True))):
        ff = g.fresh(owner=any_owner(), tag=0xFFFFFFFF)
        fe = ff.copy()
        fe[8:12] = np.frombuffer(np.uint32(0xFFFFFFFE).tobytes(), np.uint8)
        first = True
        for d, have in ((fe, fe_row), (ff, ff_row)):  # the fe row first: the ff query passes it
            if have:
                row("tagff", d, CHUNK_SIZE, _hit_blob(k), new_group=first)
                first = False
            q("q_tagff" if have else "m_tagff", d)
    # boundary prefixes, both sides, and the two ends
    for p in sorted({0, 0xFFFF} | {x for b in boundaries(W) for x in (b - 1, b)}):
        o = (p * W) >> 16
        if o in populated:
            d = g.fresh(prefix=p)
            row("boundary", d, CHUNK_SIZE, _hit_blob(p), new_group=False)
            q("q_boundary", d)
        q("m_boundary", g.fresh(prefix=p))
    # the size rule
    d = g.fresh(owner=any_owner())
    row("wildcard", d, 0, 2)
    q("q_wildcard", d, 12345)
    sz = g.fresh(owner=any_owner())
    row("sizerule", sz, S1, 0)
    for k, length in enumerate((S2, S2, S1)):
        q("q_sizerule", sz, length, order=k)
    dup = g.fresh(owner=any_owner())
    r0 = row("duprow", dup, 0, 4)
    row("duprow", dup, CHUNK_SIZE, DUP_BLOB, after=r0, new_group=False)
    q("q_duprow", dup)
    for b in UNHIT_BLOBS + UNHIT_BLOBS:
        row("unhit", g.fresh(owner=any_owner()), CHUNK_SIZE, b, new_group=False)
    for j in range(5 * W + 12):
        d = g.fresh(owner=any_owner())
        row("plain", d, (CHUNK_SIZE, CHUNK_SIZE, 0, CHUNK_SIZE, 4096)[j % 5], _hit_blob(j), new_group=False)
        q("q_plain", d)
    # empty parts are asked too
    for o in range(W):
        if o not in populated:
            for _ in range(3):
                q("m_empty", g.fresh(owner=o))
    # per part: the wrapping chain, homed at the cap the part has with these rows in
    own = dc.owner_of(np.stack([r[0] for r in rows]), W)
    for o in populated:
        cap = part_cap(int((own == o).sum()) + WRAP)
        ws = g.words_homed(o, cap - 2, cap - 1, WRAP)
        for j, w in enumerate(ws):
            d = g.fresh(words=w)
            row("part_wrap", d, CHUNK_SIZE, _hit_blob(j + 1), new_group=(j == 0))
            q("q_part_wrap", d)
        q("m_wrap", g.fresh(words=ws[0]))
    # table order: shuffled, a repeat after the row it repeats
    m = len(rows)
    order = [int(x) for x in g.rng.permutation(m)]
    at = {r: k for k, r in enumerate(order)}
    for r in range(m):
        a = rows[r][4]
        if a is not None and at[r] < at[a]:
            order[at[r]], order[at[a]] = a, r
            at[r], at[a] = at[a], at[r]
    new_id = {r: k for k, r in enumerate(order)}
    dd = np.stack([rows[r][0] for r in order])
    ds = np.array([rows[r][1] for r in order], np.uint32)
    db = np.array([rows[r][2] for r in order], np.uint32)
    di = (1000 + 3 * np.arange(m)).astype(np.uint32)
    duoff = (np.arange(m, dtype=np.uint64) + 1) * np.uint64(0x123456000)
    row_classes = {c: [np.array([new_id[r] for r in grp], np.int64) for grp in gs] for c, gs in classes.items()}
    return NodeDict(f"W{W}-{variant}", W, variant, (dd, ds, db, di, duoff, N_BLOBS), row_classes, queries)


def build_layer(nd, n, kind="mixed", seed=SEED):
    """A layer of n chunks over node dict nd -> dedup_cases.Case (its .dict is
    nd.rows).  The crafted queries come first in a round over the classes (all
    of them fit from n = 257 up), then plain hits, fresh misses and repeats."""
    W = nd.W
    g = _Gen(W, seed, 100 + 10 * n + KINDS.index(kind) + 1000 * VARIANTS.index(nd.variant))
    g.ctr = 1 << 40  # tails never equal a dict builder's

    def allowed(d):
        o = int(dc.owner_of(d[None], W)[0])
        return o == W - 1 if kind == "one" else o != 0 if kind == "avoid" else True

    def owner_pick():
        return W - 1 if kind == "one" else int(g.rng.integers(1 if kind == "avoid" and W > 1 else 0, W))

    by_class = {}
    for cls, d, length, order in nd.queries:
        if allowed(d):
            by_class.setdefault(cls, []).append((cls, d, length, order))
    items = []
    lists = list(by_class.values())
    k = 0
    while len(items) < n and any(lists):
        for lst in lists:
            if k < len(lst) and len(items) < n:
                items.append(lst[k])
        k += 1
        if all(k >= len(lst) for lst in lists):
            break
    rows_ok = [j for j in range(nd.m) if allowed(nd.rows[0][j]) and int(nd.rows[2][j]) not in UNHIT_BLOBS]
    while len(items) < n:
        t = len(items) % 8
        if t < 3 and rows_ok:
            j = rows_ok[int(g.rng.integers(0, len(rows_ok)))]
            items.append(("q_plain", nd.rows[0][j], CHUNK_SIZE, None))
        elif t == 7 and len(items) > 4:
            c, d, length, o = items[int(g.rng.integers(0, len(items)))]
            if o is not None:  # the size rule's chunks stay three
                d, length = g.fresh(owner=owner_pick()), CHUNK_SIZE
            items.append(("intra" if o is None else "m_plain", d, length, None))
        else:
            length = CHUNK_SIZE if g.rng.integers(0, 4) else int(g.rng.integers(1, CHUNK_SIZE + 1))
            items.append(("m_plain", g.fresh(owner=owner_pick()), length, None))
    pos = g.rng.permutation(n)
    fixed = [i for i, it in enumerate(items) if it[3] is not None]
    if fixed:  # the size rule's chunks keep their order
        fixed.sort(key=lambda i: items[i][3])
        pos[fixed] = np.sort(pos[fixed])
    digests = np.zeros((n, 32), np.uint8)
    lengths = np.zeros(n, np.uint32)
    classes = {}
    for i, (cls, d, length, _) in enumerate(items):
        digests[pos[i]], lengths[pos[i]] = d, length
        classes.setdefault(cls, [[]])[0].append(int(pos[i]))
    classes = {c: [np.array(sorted(gs[0]) if c != "q_sizerule" else gs[0], np.int64)] for c, gs in classes.items()}
    return dc.Case(f"{nd.name}-{kind}{n}", digests, lengths, nd.rows, classes, 4096)


# ---- dict extend: three segments per part ---------------------------------------
class ExtendCase:
    """segs: three (dd, ds, db, di, duoff) row blocks (d0 = create(segs[0]),
    d1 = extend(d0, segs[1]), d2 = extend(d1, segs[2])); q: the query digests;
    pm0 / k1 / k2: rows per part of each segment; cap1: the table capacity per
    part of the storage d1 forks onto (dict_grow_plan), where the wrap rows of
    all three segments are homed at cap1 - 2."""


def fork_caps(m, k):
    """dict_grow_plan's fork: record and table capacity for m + k entries."""
    n = m + k
    want = n + max(k, n // 2)
    return want, part_cap(want)


def build_extend(W, seed=SEED):
    g = _Gen(W, seed, 77)
    # rows per part and segment: (chain members, wrap rows, plain); the last part
    # of W >= 3 owns nothing until the first extend
    plan = [(3, 2, 10), (2, 2, 6), (2, 2, 1)]
    late = W - 1 if W >= 3 else None
    ex = ExtendCase()
    ex.W = W
    ex.pm0 = [0 if o == late else sum(plan[0]) for o in range(W)]
    ex.k1 = [sum(plan[1])] * W
    ex.k2 = [sum(plan[2]) + 3] * W  # + three repeats of d1's digests
    ex.cap1 = [fork_caps(m, k)[1] for m, k in zip(ex.pm0, ex.k1)]
    for o in range(W):  # the second extend lands in place on every part
        cap_r, cap_t = fork_caps(ex.pm0[o], ex.k1[o])
        assert ex.pm0[o] + ex.k1[o] + ex.k2[o] <= cap_r and 2 * (ex.pm0[o] + ex.k1[o] + ex.k2[o]) + 16 <= cap_t
    segs = [[], [], []]
    ex.chain, ex.wrap, ex.repeats, miss = {}, {}, [], []
    for o in range(W):
        head = g.fresh(owner=o, tag=int(g.rng.integers(0, 0xFFFFFFF0)))[:12].copy()
        ws = g.words_homed(o, ex.cap1[o] - 2, ex.cap1[o] - 1, sum(p[1] for p in plan))
        ex.chain[o], ex.wrap[o] = [], []
        for s, (nc, nw, npl) in enumerate(plan):
            if s == 0 and o == late:
                continue
            for _ in range(nc):
                d = g.fresh(head12=head)
                if s == 2 and len(ex.chain[o]) and not any(x[0] == 2 for x in ex.chain[o]):
                    d = ex.chain[o][-1][1].copy()  # a near-twin of d1's last chain row
                    d[31] ^= 0x01
                ex.chain[o].append((s, d))
                segs[s].append(d)
            for _ in range(nw):
                d = g.fresh(words=ws.pop())
                ex.wrap[o].append((s, d))
                segs[s].append(d)
            for _ in range(npl):
                segs[s].append(g.fresh(owner=o))
        # the in-place append repeats d1's digests: a chain row, a wrap row, a plain row
        olds = [next(d for s, d in ex.chain[o] if s == 1), next(d for s, d in ex.wrap[o] if s == 1),
                segs[1][-1]]
        for d in olds:
            ex.repeats.append(d)
            segs[2].append(d)
        miss += [g.fresh(head12=head), g.fresh(words=int(np.ascontiguousarray(ex.wrap[o][0][1][:8]).view("<u8")[0])),
                 g.fresh(owner=o)]
    ex.segs = []
    base = 0
    for s in range(3):
        order = g.rng.permutation(len(segs[s]))
        dd = np.stack([segs[s][int(i)] for i in order])
        k = len(dd)
        ex.segs.append((dd, np.full(k, CHUNK_SIZE, np.uint32), (np.arange(k) % 3).astype(np.uint32),
                        (5000 + 7 * (base + np.arange(k))).astype(np.uint32),
                        (np.arange(k, dtype=np.uint64) + base + 1) * np.uint64(0x1000)))
        base += k
    allrows = np.concatenate([s[0] for s in ex.segs])
    uniq = list({bytes(x): x for x in allrows}.values())
    q = uniq + miss
    ex.q = np.stack([q[int(i)] for i in g.rng.permutation(len(q))])
    ex.n_miss = len(miss)
    return ex


_CACHE = {}


def get_dict(W, variant="full"):
    key = (W, variant)
    if key not in _CACHE:
        _CACHE[key] = build_dict(W, variant)
    return _CACHE[key]


def get_layer(W, variant, n, kind="mixed"):
    key = (W, variant, n, kind)
    if key not in _CACHE:
        _CACHE[key] = build_layer(get_dict(W, variant), n, kind)
    return _CACHE[key]


def get_extend(W):
    key = ("extend", W)
    if key not in _CACHE:
        _CACHE[key] = build_extend(W)
    return _CACHE[key]
