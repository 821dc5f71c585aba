"""Ragged layers for the BLAKE3 load-mode x leaf-group matrix
(test_gpu_b3_matrix.py), and the plan those layers get, restated in numpy.

A plain helper: two deterministic builders, each returning (data_bytes,
chunks) with chunks in nydus_gpu.CHUNK_DTYPE, and plan_counts().  The
conditions that make the GPU matrix mean something (which planner and leaf
kernel a layer selects, how many chunks take each branch of b3_groups<D>) are
asserted on the CPU by test_b3_shapes.py.
"""
import numpy as np

import nydus_gpu

KIB = 1024
LEAF = 1024          # a BLAKE3 chunk: one "leaf" of the kernels
WINDOW_LOG2 = 8      # b3_groups: 256 leaf groups per workgroup window

A_CHUNK_SIZE = 0x1000000
B_CHUNK_SIZE = 0x10000
A_SEED = 20240531
B_SEED = 20240607

BLOCK_EDGES = [1, 55, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
GROUP_KIB = [1, 2, 4, 8, 16]   # the bytes of one leaf group at D = 0 .. 4
A_RUN = 400                    # the closing run of whole 64 KiB chunks
A_LAST = 37 * KIB + 5


def _place(rng, items):
    """items: (length, how) in order, how = "aligned" (the offset is padded up
    to a multiple of 16), "odd" (a gap of 1..15 bytes that leaves the offset
    odd) or an int (that many gap bytes).  -> (offsets, end)."""
    offs, pos = [], 0
    for length, how in items:
        if how == "aligned":
            pos = (pos + 15) & ~15
        elif how == "odd":
            gap = int(rng.integers(1, 16))
            if (pos + gap) % 2 == 0:
                gap += 1 if gap < 15 else -1
            pos += gap
        else:
            pos += int(how)
        offs.append(pos)
        pos += int(length)
    return offs, pos


def _finish(rng, items, offs, end, dups):
    """Random bytes (the gaps too), then the planted duplicates: chunk i takes
    the bytes of chunk j (same length), so the dedup decisions have INTRA rows."""
    data = rng.integers(0, 256, end, dtype=np.uint8)
    ch = np.zeros(len(items), nydus_gpu.CHUNK_DTYPE)
    ch["offset"] = offs
    ch["length"] = [l for l, _ in items]
    ch["file_index"] = np.arange(len(items))
    for i, j in dups:
        assert ch["length"][i] == ch["length"][j] and j < i
        o, s, n = int(ch["offset"][i]), int(ch["offset"][j]), int(ch["length"][i])
        data[o:o + n] = data[s:s + n]
    return data.tobytes(), ch


def layer_a():
    """~46 MiB, ~1,400 chunks, engine chunk_size = A_CHUNK_SIZE."""
    rng = np.random.default_rng(A_SEED)
    items = [(l, ("aligned", "odd")[i & 1]) for i, l in enumerate(BLOCK_EDGES)]
    # exactly one, two and three groups of every D, +- one byte, both alignments
    for g in GROUP_KIB:
        for m in (1, 2, 3):
            for d in (-1, 0, 1):
                items += [(m * g * KIB + d, "aligned"), (m * g * KIB + d, "odd")]
    items.append((1025 * KIB + 1, "aligned"))    # D = 0: > 1,024 group CVs, two wide tiles
    items.append((257 * 16 * KIB + 1, "odd"))    # > 256 groups at every D: never one window
    for i, l in enumerate(rng.integers(1, 48 * KIB + 1, 600)):
        items.append((int(l), ("aligned", "odd")[i & 1]))
    items += [(int(l), 0) for l in rng.integers(1, KIB + 1, 300)]
    items = [items[i] for i in rng.permutation(len(items))]
    first_run = len(items)
    items += [(64 * KIB, "aligned")] * A_RUN
    items.append((A_LAST, "aligned"))            # ends with the buffer: no padding after it
    offs, end = _place(rng, items)
    dups = [(first_run + i, first_run + i - 3) for i in range(7, A_RUN, 40)]
    return _finish(rng, items, offs, end, dups)


def layer_b():
    """~17 MiB, exactly 4,500 chunks, engine chunk_size = B_CHUNK_SIZE."""
    rng = np.random.default_rng(B_SEED)
    lens = np.concatenate([rng.integers(1, 4 * KIB + 1, 4200), rng.integers(1, 64 * KIB + 1, 300)])
    lens = lens[rng.permutation(len(lens))]
    dups = []
    for i in range(100, len(lens), 90):  # 49 planted duplicates of the chunk 37 before
        lens[i] = lens[i - 37]
        dups.append((i, i - 37))
    items = [(int(l), "aligned" if i % 2 == 0 else int(rng.integers(0, 4)))
             for i, l in enumerate(lens)]
    offs, end = _place(rng, items)
    return _finish(rng, items, offs, end, dups)


def plan_counts(chunks, D):
    """(single-group, in-window, window-straddling) chunk counts of the plan at
    2^D leaves per group: a chunk of <= 2^D leaves is one lane's work; the
    others have ceil(leaves / 2^D) groups at bases that are the prefix sum over
    them in chunk order, and finish inside one b3_groups workgroup when all
    their groups lie in one 256-group window (else they go to b3_tree)."""
    ln = np.asarray(chunks["length"], dtype=np.int64)
    leaves = np.maximum(1, (ln + LEAF - 1) // LEAF)
    multi = leaves > (1 << D)
    groups = np.where(multi, (leaves + (1 << D) - 1) >> D, 0)
    base = np.cumsum(groups) - groups
    inwin = multi & ((base >> WINDOW_LOG2) == ((base + groups - 1) >> WINDOW_LOG2))
    return int((~multi).sum()), int(inwin.sum()), int((multi & ~inwin).sum())
