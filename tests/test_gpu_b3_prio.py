"""compress() (csrc/b3_compress.hpp) flips the wave's priority between its
4-cycle and 2-cycle runs.  s_setprio ignores EXEC, and compress() is called
from divergent code: the per-lane merge loop of finish() and the comp branches
of b3_tree.  One layer whose waves mix every control path around the flips,
digests and dedup decisions bit-exact against the CPU oracle, at 1 and 8
leaves per lane under the fused and the grid planner.  Run on a gfx950 box:
pytest -m gpu."""
import numpy as np
import pytest

import nydus_gpu

pytestmark = pytest.mark.gpu

KIB = 1024
CHUNK_SIZE = 0x100000
GRID = nydus_gpu.FLAG_GRID_STAGES
DEDUP_FIELDS = ("kind", "index", "ref", "uncompressed_offset")
QUAD_MAX_LEAVES = 40960   # at or below it one leaf per lane runs compress_quad, not compress()
WINDOW_LOG2 = 8           # b3_groups: 256 leaf groups per workgroup window

# interleaved, so the 64 lanes of a wave hold leaves of every kind: one block,
# a whole leaf, a leaf and a byte, a ragged 4-leaf chunk, a full 8-leaf group,
# a full group plus a one-leaf group (merge depths differ inside the wave),
# and a chunk of 9 groups
PATTERN = [1, KIB, KIB + 1, 3 * KIB + 7, 8 * KIB, 8 * KIB + 1, 65 * KIB]
REPS_BEFORE_BIG, REPS_AFTER_BIG = 20, 4
BIG = 300 * KIB + 5       # general loop, straddles a window, goes to b3_tree
FILL = 40                 # whole 1 MiB chunks: past QUAD_MAX_LEAVES, the flagship's shape


def _layer():
    rng = np.random.default_rng(20250117)
    lens, big_at, empty_at = [], None, None
    for r in range(REPS_BEFORE_BIG + REPS_AFTER_BIG):
        if r == REPS_BEFORE_BIG:
            big_at = len(lens)
            lens.append(BIG)
        for k, l in enumerate(PATTERN):
            lens.append(l)
            if r == 7 and k == 3:
                empty_at = len(lens)
                lens.append(0)
    lens += [CHUNK_SIZE] * FILL
    offs, pos = [], 0
    for i, l in enumerate(lens):
        if i == big_at:
            pos = ((pos + 15) & ~15) + 5       # not 16-B aligned
        elif i % 3 == 0:
            pos = (pos + 15) & ~15
        elif i % 3 == 1:
            pos += 3
        offs.append(pos)
        pos += l
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    ch = np.zeros(len(lens), nydus_gpu.CHUNK_DTYPE)
    ch["offset"], ch["length"] = offs, lens
    ch["file_index"] = np.arange(len(lens))
    # planted duplicates: a repetition's chunks of 1,025 B, 8,193 B and 65 KiB
    # repeat the bytes of the same chunk two repetitions earlier
    first = {}
    for i, l in enumerate(lens):
        if l in (KIB + 1, 8 * KIB + 1, 65 * KIB):
            seen = first.setdefault(l, [])
            if len(seen) >= 2 and len(seen) % 4 >= 2:
                s, o = int(ch["offset"][seen[-2]]), offs[i]
                data[o:o + l] = data[s:s + l]
            seen.append(i)
    return data.tobytes(), ch, big_at, empty_at


@pytest.fixture(scope="module")
def ref(oracle):
    data, ch, big_at, empty_at = _layer()
    assert ch["length"][empty_at] == 0 and ch["offset"][big_at] % 16 == 5
    assert len(data) // KIB + len(ch) > QUAD_MAX_LEAVES     # b3_groups<0>, not the quad kernels
    assert int(ch["length"].max()) <= CHUNK_SIZE
    leaves = np.maximum(1, (ch["length"].astype(np.int64) + KIB - 1) // KIB)
    for D in (0, 3):  # the big chunk's groups cross a window at both group sizes
        groups = np.where(leaves > (1 << D), (leaves + (1 << D) - 1) >> D, 0)
        base = int(groups[:big_at].sum())
        assert base >> WINDOW_LOG2 != (base + int(groups[big_at]) - 1) >> WINDOW_LOG2, D
    dig = oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), "blake3")
    dec, _ = oracle.dedup(dig, ch["length"])
    assert (dec["kind"] == nydus_gpu.INTRA).sum() >= 20
    for a in (ch, dig, dec):
        a.setflags(write=False)
    return data, ch, dig, dec


@pytest.mark.parametrize("flags", [0, GRID], ids=["fused", "grid"])
@pytest.mark.parametrize("lanes", [1, 8])
def test_mixed_wave_vs_oracle(ref, lanes, flags):
    data, ch, dig, dec = ref
    with nydus_gpu.Engine(digester="blake3", chunk_size=CHUNK_SIZE, leaves_per_lane=lanes,
                          flags=flags) as eng:
        out, st = eng.process(data, ch)
    bad = np.nonzero((out["digest"] != dig).any(axis=1))[0]
    assert bad.size == 0, (f"digest: {bad.size} bad chunks, first ids={bad[:8].tolist()} "
                           f"lengths={ch['length'][bad[:8]].tolist()}")
    for f in DEDUP_FIELDS:
        bad = np.nonzero(out[f] != dec[f])[0]
        assert bad.size == 0, f"{f}: {bad.size} bad chunks, first ids={bad[:8].tolist()}"
    assert st["chunks"] == len(ch)
