"""Layers for the SHA-256 dispatch matrix (test_gpu_sha_matrix.py), and the
kernel selection rule of csrc/sha256_plan.hpp restated in Python.

A plain helper: three deterministic builders, each returning (data_bytes,
chunks) with chunks in nydus_gpu.CHUNK_DTYPE, and the mirror sha_mixed /
sha_pick / pick_name.  The conditions that make the GPU matrix mean something
(which of the seven kernels a (layer, form, prefix, flag) runs, which padding
edges meet which lane positions) are asserted on the CPU by test_sha_shapes.py,
which also ties the mirror to the header's own picks.

Every builder takes `pad`.  pad=True inserts a gap of unused random bytes before
the last group of 32 chunks, long enough that sha_mixed is false; pad=False does
not.  Chunk lengths and contents are the same either way (so are the digests),
only the offsets differ, by a multiple of 16; in both forms the last chunk ends
with the buffer.
"""
import hashlib
import os
import subprocess

import numpy as np

import nydus_gpu

SHA_MODE_SHIFT = 11   # NGPU_FLAG_SHA_MODE_SHIFT: bits 11..13 = 1 + variant
VARIANT_FLAGS = [0, 1 << 11, 2 << 11, 3 << 11, 5 << 11, 6 << 11]
KERNELS = ["split", "lane", "pair<1,U>", "pair<1,M>", "pair<2,U>", "pair<2,M>", "pair<4,M>"]

E_CHUNK_SIZE = 0x1000
R_CHUNK_SIZE = 0x10000
C_CHUNK_SIZE = 0x1000
E_SEED, R_SEED, C_SEED = 20250114, 20250121, 20250128
E_CHUNKS, R_CHUNKS, C_CHUNKS = 960, 224, 32769
E_MAX_LEN = 320
R_PREFIXES = [1, 33, 223]
C_PREFIXES = [16384, 16385, 32768, 32769]
R_LONG = 65536                 # 1025 blocks
R_G1_LONG_AT = 13
R_G5_LONG_AT = (7, 8, 31)      # both sides of a DPP row boundary, and the last lane pair


def build_plan_test(exe):
    """Compile tests/cpp/sha256_plan_test.cpp (the header's rule, stand-alone,
    under ASan/UBSan) to `exe`."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "sha256_plan_test.cpp"), "-o", exe])
    return exe


# ---- the rule (csrc/sha256_plan.hpp) ----------------------------------------------

def sha_mixed(n, length, chunk_size):
    return n % 32 != 0 or length < n * chunk_size // 16 * 15


def variant_of(flags):
    sv = (flags >> SHA_MODE_SHIFT) & 7
    return sv - 1 if sv else -1


def sha_pick(variant, n, mixed):
    """-> dict(name, R, chunks_per_wg, threads, grid)."""
    if variant < 0:
        variant = 1 if n <= 16384 else 5 if n <= 32768 else 2
    if variant == 0:
        name, R, per, threads = "split", 0, 64, 128
    elif variant == 2:
        name, R, per, threads = "lane", 0, 256, 256
    else:
        R = {4: 1, 5: 4}.get(variant, 2)
        name = f"pair<{R},{'U' if R != 4 and mixed else 'M'}>"
        per, threads = 32 * R, 128 * R
    return {"name": name, "R": R, "chunks_per_wg": per, "threads": threads, "grid": -(-n // per)}


def pick_name(flags, n, length, chunk_size):
    """The kernel a digest call of n chunks over a `length`-byte buffer runs."""
    return sha_pick(variant_of(flags), n, sha_mixed(n, length, chunk_size))["name"]


def blocks_of(lengths):
    """SHA-256 blocks of a message: data, 0x80, zero pad, 8 length bytes."""
    return (np.asarray(lengths, dtype=np.int64) + 8) // 64 + 1


def tail_class(length):
    r = int(length) % 64
    return "Z" if r == 0 else "T1" if r <= 55 else "T2"


def hashlib_digests(data, ch):
    """The reference: hashlib.sha256 over every chunk's bytes."""
    mv = memoryview(data)
    out = np.zeros((len(ch), 32), np.uint8)
    for i, (o, l) in enumerate(zip(ch["offset"].tolist(), ch["length"].tolist())):
        out[i] = np.frombuffer(hashlib.sha256(mv[o:o + l]).digest(), np.uint8)
    return out


# ---- builders ----------------------------------------------------------------------

def _build(rng, items, dups, pad, chunk_size):
    """items: (length, how) in chunk order, how = "A" (the offset is padded up
    to a multiple of 16) or "O" (a gap of 1..15 bytes that leaves the offset
    odd) or "B" (back to back).  dups: (i, j), chunk i takes the bytes of chunk
    j < i of the same length.  All random draws are the same in both forms."""
    n = len(items)
    offs, pos = [], 0
    for length, how in items:
        if how == "A":
            pos = (pos + 15) & ~15
        elif how == "O":
            pos += int(rng.integers(0, 8)) * 2 + (1 if pos % 2 == 0 else 2)
        offs.append(pos)
        pos += int(length)
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    filler = rng.integers(0, 256, n * chunk_size // 16 * 15 + 16, dtype=np.uint8) if pad else None
    ch = np.zeros(n, nydus_gpu.CHUNK_DTYPE)
    ch["offset"] = offs
    ch["length"] = [l for l, _ in items]
    ch["file_index"] = np.arange(n)
    for i, j in dups:
        assert ch["length"][i] == ch["length"][j] and j < i
        o, s, l = int(ch["offset"][i]), int(ch["offset"][j]), int(ch["length"][i])
        data[o:o + l] = data[s:s + l]
    if pad:
        first = (n - 1) // 32 * 32          # the last group of 32 (or what there is of it)
        cut = int(ch["offset"][first])
        need = n * chunk_size // 16 * 15 - len(data)
        gap = max(0, (need + 15) & ~15)     # a multiple of 16: every offset % 16 is kept
        data = np.concatenate([data[:cut], filler[:gap], data[cut:]])
        ch["offset"][first:] += gap
    return data.tobytes(), ch


def _dups_by_length(lengths, wanted):
    """For each id in `wanted`: (i, j) with i the first chunk at or after it
    that has an earlier chunk of its length, and j the nearest such chunk that
    is not itself a copy."""
    out, used = [], set()
    for w in wanted:
        for i in range(w, len(lengths)):
            js = [j for j in range(i - 1, -1, -1) if lengths[j] == lengths[i] and j not in used]
            if js and i not in used:
                out.append((i, js[0]))
                used.add(i)
                break
        else:
            raise ValueError(f"no chunk from {w} on repeats an earlier length")
    return out


E_COMBOS = [(t, a) for t in ("T1", "T2", "Z") for a in ("A", "O")]


def layer_e(pad):
    """Edges x positions: 960 chunks of 1..320 bytes (1..6 blocks).  Chunk i
    (group g = i // 32, position p = i % 32) is of tail class x alignment
    E_COMBOS[(g + p) % 6], so every position sees every combination five times;
    every length 1..320 occurs."""
    rng = np.random.default_rng(E_SEED)
    pools = {c: [l for l in range(1, E_MAX_LEN + 1) if tail_class(l) == c] for c in ("T1", "T2", "Z")}
    order = {c: [] for c in pools}
    items = []
    for i in range(E_CHUNKS):
        t, a = E_COMBOS[(i // 32 + i % 32) % 6]
        if not order[t]:  # each pass over a class takes every length of it once, shuffled
            order[t] = [pools[t][k] for k in rng.permutation(len(pools[t]))]
        items.append((order[t].pop(), a))
    lengths = [l for l, _ in items]
    dups = _dups_by_length(lengths, [300, 301, 517, 640, 911, 930])
    return _build(rng, items, dups, pad, E_CHUNK_SIZE)


def layer_r(pad):
    """Ragged chains: seven groups of 32, the longest chain 1025 blocks."""
    rng = np.random.default_rng(R_SEED)
    items = [(R_LONG, "A")] * 32                                              # g0
    g1 = [int(l) for l in rng.integers(1, 201, 32)]
    g1[R_G1_LONG_AT] = R_LONG
    items += [(l, ("A", "O")[k & 1]) for k, l in enumerate(g1)]              # g1
    g2 = [int(l) for l in rng.integers(1, 56, 32)]
    g2[20] = g2[3]
    items += [(l, ("O", "A")[k & 1]) for k, l in enumerate(g2)]              # g2
    items += [(int(l), "O") for l in rng.integers(1, R_LONG + 1, 32)]         # g3
    for p in range(32):                                                       # g4
        nb = 1 + 7 * (31 - p)                  # 218, 211, ... 8, 1 blocks
        lo, hi = max(1, 64 * (nb - 1) - 8), 64 * (nb - 1) + 55
        items.append((int(rng.integers(lo, hi + 1)), ("A", "O")[p & 1]))
    for p in range(32):                                                       # g5
        long = p in R_G5_LONG_AT
        items.append((int(rng.integers(20000, R_LONG + 1) if long else rng.integers(1, 201)),
                      ("A", "O")[(p >> 1) & 1]))
    items += [(int(l), "A") for l in rng.integers(1, R_LONG + 1, 32)]         # g6
    # g0 copies inside g0, g1's long chunk a copy of g0's first, a one-block pair in g2
    dups = [(5, 2), (17, 16), (31, 30), (32 + R_G1_LONG_AT, 0), (64 + 20, 64 + 3)]
    return _build(rng, items, dups, pad, R_CHUNK_SIZE)


def layer_c(pad=False):
    """Counts: 32,769 chunks of 1..200 bytes, back to back.  Its calls are mixed
    in every form (a padded one would need 126 MB, and 32,769 is no multiple of
    32), so only pad=False is built."""
    if pad:
        raise ValueError("layer C has no padded form")
    rng = np.random.default_rng(C_SEED)
    lengths = [int(l) for l in rng.integers(1, 201, C_CHUNKS)]
    items = [(l, "B") for l in lengths]
    dups = _dups_by_length(lengths, [5000, 16383, 16384, 20000, 32767, 32768])
    return _build(rng, items, dups, False, C_CHUNK_SIZE)


LAYERS = {"E": (layer_e, E_CHUNK_SIZE), "R": (layer_r, R_CHUNK_SIZE), "C": (layer_c, C_CHUNK_SIZE)}


def matrix_calls():
    """Every digest call of test_gpu_sha_matrix.py as (layer, pad, n, flags):
    n chunks (a prefix, or all) of the layer's form over its whole buffer."""
    calls = []
    for layer, n in (("E", E_CHUNKS), ("R", R_CHUNKS)):
        for pad in (True, False):
            calls += [(layer, pad, n, f) for f in VARIANT_FLAGS]
    calls += [("R", False, n, f) for n in R_PREFIXES for f in VARIANT_FLAGS]
    calls += [("C", False, n, 0) for n in C_PREFIXES]
    calls += [("C", False, C_CHUNKS, f) for f in VARIANT_FLAGS[1:]]
    return calls
