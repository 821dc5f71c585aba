"""Crafted digests for the dedup collision matrix (test_dedup_cases.py on the
CPU, test_gpu_dedup_collisions.py on the GPU).

A plain helper: numpy only, every generator seeded, nothing imported from the
GPU library.  The dedup stage never looks at a chunk's bytes, only at its
32-byte digest and its length, so a case is a digest array and a length array
(plus the chunk dict's rows) and reaches the kernels through records marked
NGPU_DIGESTED -- no byte is hashed.

A digest as csrc/dict_hash.hpp reads it:
  bytes 0-7    the bucket words (digest_bucket: their u64 times the golden
               ratio, folded once and masked to the table size, is the home
               slot: home_slot below, tied to the header by test_dict_hash.py)
  bytes 8-11   the tag (digest_tag: word 2, 0xFFFFFFFF stored as 0xFFFFFFFE)
  bytes 12-31  the tail: bytes 12-15 a group word (equal inside a tagchain
               group, so bytes 8-15 -- the key of oracle/dedup_ref.c's own
               table -- collide there too), bytes 16-23 a counter that makes
               every fresh digest distinct and non-zero, bytes 24-31 random.

Classes (Case.classes maps a name to a list of groups of chunk ids):
  tagchain     k digests sharing bytes 0-15; member 1 differs from member 0
               only in byte 31; repeats of members 0 and 1 lie around them
  bucketchain  equal bytes 0-7, different tags
  slotchain    different bucket words, one home slot of the single-layer LDS
               table (lds_mask(n)); the first chain is homed at mask - 2 and
               wraps to slot 0
  tagff        equal bucket words and tails, tags 0xFFFFFFFF / 0xFFFFFFFE,
               and a true duplicate of each: [ff, fe, ff again, fe again]
  sizerule     one digest at lengths (S1, S2, S2) and one at (S1, S1, S2, S1)
  hot          one digest on >= n / 4 chunks, chunk 0 never among them
  lengths      [the chunks of 1, 4095, 4096, 4097 bytes], [the 16 MiB chunks]
  plain        well-distributed digests, a few of them repeated
  dict_*       see _Builder.dict_classes

Lengths are always >= 1 and no digest is all zero (the unwritten-digest
guard's state).  The oracle's `sizes[l] == 0` wildcard for zero-length chunks
of the layered dict is out of scope: no case has a zero-length chunk.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15  # digest_bucket's multiplier (dict_hash.hpp)
CHUNK_SIZE = 0x1000000       # the engine's chunk size in these tests: 16 MiB
S1, S2 = CHUNK_SIZE, CHUNK_SIZE - 4095
EDGE_LENGTHS = (1, 4095, 4096, 4097)
N_BLOBS = 16
MANY_BLOBS = 1100            # > 1023 dict blobs: one layer leaves the LDS kernel
HIT_BLOBS = (15, 13, 11, 9, 7, 5, 3, 1, 2, 0, 8, 12)  # inner blobs 4, 6, 10, 14: never hit


def lds_mask(n):
    """The table mask dedup_small_lds uses for a layer of n chunks."""
    mask = 63
    while mask + 1 < 2 * n:
        mask = mask * 2 + 1
    return mask


def word_slot(words, mask):
    """Home slot of u64 bucket words: the product folded once (x ^ x >> 32),
    masked.  The one Python statement of digest_bucket; test_dict_hash.py ties
    it to the header."""
    x = np.multiply(np.asarray(words, np.uint64), np.uint64(GOLDEN))
    return (x ^ (x >> np.uint64(32))) & np.uint64(mask)


def home_slot(digests, mask):
    """digest_bucket(d) & mask for an (n, 32) u8 array."""
    return word_slot(np.ascontiguousarray(digests[:, :8]).view("<u8")[:, 0], mask)


def tag_of(digests):
    """digest_tag(d) for an (n, 32) u8 array: word 2, 0xFFFFFFFF as 0xFFFFFFFE."""
    t = np.ascontiguousarray(digests[:, 8:12]).view("<u4")[:, 0].copy()
    t[t == 0xFFFFFFFF] = 0xFFFFFFFE
    return t


def owner_of(digests, W):
    """The node owner of each digest of an (n, 32) u8 array (dist.owner_of's
    rule; test_dict_hash.py holds the statements together)."""
    hi = digests[:, 0].astype(np.int64) << 8 | digests[:, 1].astype(np.int64)
    return (hi * W) >> 16


def lds_thread_wave(n, c):
    """(thread, wave) that resolves chunk c in phase B of dedup_small_lds:
    T = 256 threads up to 256 chunks, else 1024; thread t takes the contiguous
    chunks [t R, t R + R), R = ceil(n / T)."""
    T = 256 if n <= 256 else 1024
    R = (n + T - 1) // T
    return c // R, (c // R) // 64


class Case:
    """digests (n, 32) u8, lengths (n,) u32, dict = (dd, ds, db, di, duoff,
    n_blobs) (m = 0 rows without a dict), classes, align, name."""

    def __init__(self, name, digests, lengths, dict_rows, classes, align):
        self.name, self.align = name, align
        self.digests, self.lengths = digests, lengths
        self.dict, self.classes = dict_rows, classes
        self.n = len(lengths)

    @property
    def m(self):
        return len(self.dict[1])

    def arrays(self):
        return (self.digests, self.lengths) + tuple(self.dict) + (self.classes,)


def _no_dict():
    return (np.zeros((0, 32), np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32),
            np.zeros(0, np.uint32), np.zeros(0, np.uint64), 0)


class _Builder:
    def __init__(self, n, seed, salt):
        self.n = n
        self.rng = np.random.default_rng([seed, n, salt])
        self.ctr = 0
        self.items = []      # (digest, length, class name, group number)
        self.ordered = []    # lists of item numbers whose chunk ids must ascend
        self.fixed = {}      # item number -> chunk id
        self.groups = {}     # class name -> list of lists of item numbers
        self.rows = []       # dict rows: (digest, usize, blob, index, uoff)
        self.left = n

    # -- digests ---------------------------------------------------------------
    def fresh(self, bucket=None, tag=None, grp=None):
        d = self.rng.integers(0, 256, 32, dtype=np.uint8)
        self.ctr += 1
        d[16:24] = np.frombuffer(np.uint64(self.ctr).tobytes(), np.uint8)
        if bucket is not None:
            d[0:8] = np.frombuffer(np.uint64(bucket).tobytes(), np.uint8)
        if tag is not None:
            d[8:12] = np.frombuffer(np.uint32(tag).tobytes(), np.uint8)
        if grp is not None:
            d[12:16] = np.frombuffer(np.uint32(grp).tobytes(), np.uint8)
        return d

    def word(self):
        return int(self.rng.integers(0, np.iinfo(np.uint64).max, dtype=np.uint64, endpoint=True))

    def words_for_slot(self, slot, mask, count):
        """Brute force over home_slot: `count` distinct bucket words whose
        home slot in a table of mask + 1 slots is `slot`."""
        found = []
        while len(found) < count:
            w = self.rng.integers(0, np.iinfo(np.uint64).max, 1 << 18, dtype=np.uint64, endpoint=True)
            hit = w[home_slot(w.view(np.uint8).reshape(-1, 8), mask) == np.uint64(slot)]
            found.extend(int(x) for x in hit)
        found = list(dict.fromkeys(found))[:count]
        assert len(found) == count
        return found

    # -- items -----------------------------------------------------------------
    def take(self, k):
        if k > self.left:
            return False
        self.left -= k
        return True

    def add(self, cls, members, ordered=False, new_group=True):
        """members: (digest, length) in role order -> their item numbers."""
        ids = []
        for d, length in members:
            ids.append(len(self.items))
            self.items.append((d, int(length), cls))
        g = self.groups.setdefault(cls, [])
        if new_group or not g:
            g.append([])
        g[-1].extend(ids)
        if ordered:
            self.ordered.append(list(ids))
        return ids

    def tagchain(self, k, repeats):
        """k distinct digests on one (bucket, tag, group word); member 1 is
        member 0 with byte 31 changed; repeats of 0 and 1 follow them in chunk
        order (so 0 lies before and after its near-twin 1); `repeats` - 2 more
        copies of random members anywhere."""
        b, t, g = self.word(), int(self.rng.integers(0, 0xFFFFFFF0)), int(self.rng.integers(1, 1 << 32))
        mem = [self.fresh(b, t, g) for _ in range(k)]
        mem[1] = mem[0].copy()
        mem[1][31] ^= 0x01
        ids = self.add("tagchain", [(d, CHUNK_SIZE) for d in mem])
        core = [ids[0], ids[1]] + self.add("tagchain", [(mem[0], CHUNK_SIZE)], new_group=False)
        if repeats >= 2:
            core += self.add("tagchain", [(mem[1], CHUNK_SIZE)], new_group=False)
        self.ordered.append(core)
        for _ in range(max(0, repeats - 2)):
            j = int(self.rng.integers(2, k)) if k > 2 else 0
            self.add("tagchain", [(mem[j], CHUNK_SIZE)], new_group=False)
        return mem

    # -- the mixed case ----------------------------------------------------------
    def mixed(self, with_dict, n_blobs):
        n, rng = self.n, self.rng
        mask = lds_mask(n)
        hot = -(-n // 4) if n >= 8 else 0
        self.left -= hot
        if n == 1:
            self.take(1)
            self.add("plain", [(self.fresh(), CHUNK_SIZE)])
        # tagff: [ff, fe, ff again, fe again]
        k = 4 if self.take(4) else 2 if self.take(2) else 0
        if k:
            ff = self.fresh(tag=0xFFFFFFFF)
            fe = ff.copy()
            fe[8:12] = np.frombuffer(np.uint32(0xFFFFFFFE).tobytes(), np.uint8)
            self.add("tagff", [(ff, CHUNK_SIZE), (fe, CHUNK_SIZE)] * (k // 2))
        # sizerule: members spread evenly over the layer, so that they fall in
        # different threads' runs and, from four waves of chunks up, different waves
        for lens in ((S1, S2, S2), (S1, S1, S2, S1)):
            kk = len(lens)
            where = [(2 * j + 1) * n // (2 * kk) for j in range(kk)]
            if n >= 4 * kk and not set(where) & set(self.fixed.values()) and self.take(kk):
                d = self.fresh()
                ids = self.add("sizerule", [(d, l) for l in lens])
                self.fixed.update(zip(ids, where))
        # slotchain: >= 8 distinct bucket words homed at mask - 2 (wraps to slot 0)
        edge_hosts = []
        if self.take(8):
            ws = self.words_for_slot(mask - 2, mask, 8)
            edge_hosts = self.add("slotchain", [(self.fresh(bucket=w), CHUNK_SIZE) for w in ws])
        kmax = min(48, n // 4)
        dict_chain = []
        if kmax >= 2 and self.take(kmax + 2):
            mem = self.tagchain(kmax, 2)
            dict_chain = mem[len(mem) // 2:]  # with_dict: these rows form the dict's own tagchain
        if kmax > 2 and self.take(3):
            self.tagchain(2, 1)
        if self.take(2):
            b = self.word()
            self.add("bucketchain", [(self.fresh(bucket=b), CHUNK_SIZE) for _ in range(2)])
        if with_dict:
            self.dict_classes(dict_chain, n_blobs)
        # room left: more of everything
        for k in (3, 5, 9, 17, 33):
            rep = 2 + k // 4
            if k < kmax and self.take(k + rep):
                self.tagchain(k, rep)
        if self.take(12):  # homed at the last slot: wraps at once
            ws = self.words_for_slot(mask, mask, 12)
            self.add("slotchain", [(self.fresh(bucket=w), CHUNK_SIZE) for w in ws])
        if self.take(6):
            ws = self.words_for_slot(0, mask, 6)
            self.add("slotchain", [(self.fresh(bucket=w), CHUNK_SIZE) for w in ws])
        if self.take(4):
            b = self.word()
            self.add("bucketchain", [(self.fresh(bucket=b), CHUNK_SIZE) for _ in range(4)])
        if with_dict and self.rows:
            self.dict_more(min(self.left // 4, 160), n_blobs)
        # plain: distinct digests, every eighth a repeat of an earlier plain one
        plain = []
        while self.take(1):
            if plain and len(plain) % 8 == 7:
                d, length = plain[int(rng.integers(0, len(plain)))]
            else:
                length = CHUNK_SIZE if rng.integers(0, 4) else int(rng.integers(1, CHUNK_SIZE + 1))
                d = self.fresh()
            plain.append((d, length))
            self.add("plain", [(d, length)], new_group=False)
        # hot: one digest, first seen after chunk 0
        if hot:
            d = self.fresh()
            self.add("hot", [(d, CHUNK_SIZE)] * hot)
        # lengths: the four edges go on chunks whose digest occurs once
        hosts = edge_hosts[:4] if edge_hosts else [i for i, it in enumerate(self.items) if it[2] == "plain"][:1]
        for i, l in zip(hosts, EDGE_LENGTHS):
            d, _, cls = self.items[i]
            self.items[i] = (d, l, cls)
        self.groups["lengths"] = [list(hosts[:len(EDGE_LENGTHS)])]

    def blob(self, b, n_blobs):
        """Inner blob of role b (0..15): spread over [0, n_blobs) when there are many."""
        return b if n_blobs == N_BLOBS else (b * 73 + 4 if b else 0)

    def row(self, d, usize, b, n_blobs):
        e = len(self.rows)
        self.rows.append((d, int(usize), self.blob(b, n_blobs), 1000 + 3 * e, (e + 1) * 0x123456789))
        return e

    def dict_classes(self, chain, n_blobs):
        """dict_tagchain: the upper half of the first tagchain group as dict
        rows, one blob each (their chunks hit; the dict table walks the chain);
        dict_duprow: a digest on two rows, the first a usize-0 wildcard, the
        second never answered; dict_wildcard: the chunk that hits it at an odd
        length; dict_sizerule: a row of usize S1 and chunks of (S2, S2, S1):
        refused -> NEW, INTRA to it, accepted -> DICT; dict_blobs: two more
        rows in blobs of their own.  Blobs 4, 6, 10, 14 have rows nobody hits."""
        if not chain or not self.take(6):
            return
        for b in (4, 6, 10, 14, 4):
            self.row(self.fresh(), CHUNK_SIZE, b, n_blobs)
        hit = list(HIT_BLOBS)
        self.groups["dict_tagchain"] = [[i for i, it in enumerate(self.items)
                                         if any(np.array_equal(it[0], d) for d in chain)]]
        for j, d in enumerate(chain):
            self.row(d, CHUNK_SIZE if j % 2 else 0, hit[j % 8], n_blobs)
        dup = self.fresh()
        self.row(dup, 0, 2, n_blobs)
        self.row(self.fresh(), 77, 6, n_blobs)
        self.row(dup, 12345, 4, n_blobs)  # the later row of the same digest: never the answer
        ids = self.add("dict_duprow", [(dup, 12345)])
        self.groups["dict_wildcard"] = [list(ids)]
        sz = self.fresh()
        self.row(sz, S1, 0, n_blobs)
        self.add("dict_sizerule", [(sz, S2), (sz, S2), (sz, S1)], ordered=True)
        for b in (8, 12):
            d = self.fresh()
            self.row(d, CHUNK_SIZE, b, n_blobs)
            self.add("dict_blobs", [(d, CHUNK_SIZE)], new_group=False)

    def dict_more(self, k, n_blobs):
        """k more chunks over k / 2 more rows in the blobs already hit: equal
        digests hit one row; every fifth row's usize refuses its chunks."""
        rows = []
        for j in range(max(1, k // 2)):
            d = self.fresh()
            usize = (0, CHUNK_SIZE, CHUNK_SIZE, CHUNK_SIZE, 4096)[j % 5]
            self.row(d, usize, HIT_BLOBS[int(self.rng.integers(0, len(HIT_BLOBS)))], n_blobs)
            rows.append(d)
            if j % 7 == 3:  # a second row of the same digest in another blob
                self.row(d, 0, 14, n_blobs)
        for j in range(k):
            if self.take(1):
                self.add("dict_more", [(rows[j % len(rows)], CHUNK_SIZE)], new_group=False)

    # -- placement ---------------------------------------------------------------
    def finish(self, name, align, n_blobs):
        n, rng = self.n, self.rng
        assert len(self.items) == n, (len(self.items), n)
        pos = np.full(n, -1, np.int64)
        for i, p in self.fixed.items():
            pos[i] = p
        free = [p for p in range(n) if p not in set(self.fixed.values())]
        free = [int(free[i]) for i in rng.permutation(len(free))]
        rest = [i for i in range(n) if pos[i] < 0]
        if rest and free and 0 in free:  # chunk 0 is never a hot one
            cold = next((k for k, i in enumerate(rest) if self.items[i][2] != "hot"), None)
            if cold is not None:
                z = free.index(0)
                free[z], free[cold] = free[cold], free[z]
        for i, p in zip(rest, free):
            pos[i] = p
        for grp in self.ordered:
            pos[grp] = np.sort(pos[grp])
        assert sorted(pos.tolist()) == list(range(n))
        digests = np.zeros((n, 32), np.uint8)
        lengths = np.zeros(n, np.uint32)
        for i, (d, length, _) in enumerate(self.items):
            digests[pos[i]] = d
            lengths[pos[i]] = length
        classes = {c: [pos[np.asarray(g, np.int64)] for g in gs] for c, gs in self.groups.items()}
        if "hot" in classes:
            classes["hot"] = [np.sort(classes["hot"][0])]
        if "lengths" in classes:
            classes["lengths"].append(np.flatnonzero(lengths == CHUNK_SIZE))
        if self.rows:
            dd = np.stack([r[0] for r in self.rows])
            ds, db, di = (np.array([r[k] for r in self.rows], np.uint32) for k in (1, 2, 3))
            duoff = np.array([r[4] for r in self.rows], np.uint64)
            rows = (dd, ds, db, di, duoff, n_blobs)
        else:
            rows = _no_dict()
        assert lengths.min() >= 1 and digests.any(axis=1).all()
        return Case(name, digests, lengths, rows, classes, align)


def build(n, *, with_dict, align, seed, many_blobs=False):
    """The mixed case of n chunks: every class that fits (all of them from
    n = 64 up).  many_blobs: the dict has MANY_BLOBS inner blobs, not N_BLOBS.
    -> Case: .digests, .lengths, .dict = (dd, ds, db, di, duoff, n_blobs) and
    .classes (name -> groups of chunk ids); Case.arrays() is the flat tuple."""
    n_blobs = MANY_BLOBS if many_blobs else N_BLOBS
    b = _Builder(n, seed, 1 + 2 * bool(with_dict) + 4 * bool(many_blobs))
    b.mixed(with_dict, n_blobs)
    name = f"mixed{n}" + ("-dict" if with_dict else "") + ("-many" if many_blobs else "")
    return b.finish(name, align, n_blobs if with_dict else 0)


def build_hot(n, *, align=4096, seed=1):
    """All n chunks equal: one NEW, n - 1 INTRA, every lane on one slot."""
    b = _Builder(n, seed, 101)
    d = b.fresh()
    b.take(n)
    b.add("hot", [(d, CHUNK_SIZE)] * n)
    return b.finish(f"hot{n}", align, 0)


def build_distinct(n, *, align=4096, seed=1):
    """No two chunks equal, all of 16 MiB: n = 256 totals exactly 2^32 bytes."""
    b = _Builder(n, seed, 102)
    b.take(n)
    b.add("plain", [(b.fresh(), CHUNK_SIZE) for _ in range(n)])
    return b.finish(f"distinct{n}", align, 0)


def build_all_dict(n, *, align=4096, seed=1):
    """Every chunk hits the dict (three chunks per row, usize 0 or the chunk's
    length): no NEW chunk, so the layer's own blob is never allocated."""
    b = _Builder(n, seed, 103)
    b.take(n)
    for j in range(-(-n // 3)):
        b.row(b.fresh(), 0 if j % 2 else CHUNK_SIZE, HIT_BLOBS[j % len(HIT_BLOBS)], N_BLOBS)
    b.row(b.fresh(), CHUNK_SIZE, 6, N_BLOBS)
    b.add("dict_more", [(b.rows[j // 3][0], CHUNK_SIZE) for j in range(n)])
    return b.finish(f"alldict{n}", align, N_BLOBS)


# ---- the matrix (shared by the CPU and the GPU test) ---------------------------
SEED = 20241019
PATH_N = {
    "lds256": (1, 2, 63, 64, 65, 255, 256),
    "lds1024": (257, 1023, 1024, 1025, 2049, 4095, 4096),
    "small": (64, 257, 1025, 4096),
    "grid": (1, 64, 256, 257, 1025, 4096, 4097, 6000),
}
ALL_N = tuple(sorted({n for ns in PATH_N.values() for n in ns}))
WHOLE_N = (256, 4096)  # build_hot / build_distinct / build_all_dict
_CACHE = {}


def get(kind, n, align, with_dict=False, many_blobs=False):
    """A case of the matrix, built once per process.  kind: mixed, hot,
    distinct or all_dict."""
    key = (kind, n, align, with_dict, many_blobs)
    if key not in _CACHE:
        if kind == "mixed":
            _CACHE[key] = build(n, with_dict=with_dict, align=align, seed=SEED, many_blobs=many_blobs)
        else:
            fn = {"hot": build_hot, "distinct": build_distinct, "all_dict": build_all_dict}[kind]
            _CACHE[key] = fn(n, align=align, seed=SEED)
    return _CACHE[key]
