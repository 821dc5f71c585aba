"""b3_groups keeps each lane's eager merge stack in LDS, addressed by the
lane's depth, in storage the in-window tree reuses once the leaves are done
(csrc/blake3.hip).  One layer whose chunks reach every stack depth, every
merge count and the partial last group at each leaf-group size, with lanes of
different depth in one wave, whole-leaf waves next to general-path waves, the
in-window sort running, and a window that holds both chunks finished in it and
groups of a chunk that goes to b3_tree.  Every digest against the CPU oracle,
through the C ABI, at 2, 4, 8 and 16 leaves per lane and every load mode.
Run on a gfx950 box: pytest -m gpu."""
import numpy as np
import pytest

import nydus_gpu

pytestmark = pytest.mark.gpu

KIB = 1024
CHUNK_SIZE = 0x1000000    # the largest the ABI takes: one chunk can hold more than 256 groups of 16 leaves
GRID = nydus_gpu.FLAG_GRID_STAGES
LOAD_MODES = [0, 1, 2, 3, 5]
LOAD_MODE_SHIFT = 8       # NGPU_FLAG_LOAD_MODE_SHIFT: bits 8..10 = 1 + load mode
QUAD_MAX_LEAVES = 40960   # at or below it one leaf per lane takes the quad kernels
WINDOW = 256              # b3_groups: leaf groups per workgroup window

# 1 .. 17 leaves (2^D - 1, 2^D and 2^D + 1 for D = 1 .. 4 are among them), each
# at k KiB - 1, k KiB and k KiB + 1 (the last is k + 1 leaves, one byte in the
# last), interleaved so neighbouring lanes differ in leaf count and depth
PATTERN = [k * KIB + d for k in range(1, 18) for d in (-1, 0, 1)]
REPS_BEFORE_BIG, REPS_AFTER_BIG = 7, 5
BIG = 5 * 1024 * KIB + 5  # 5,121 leaves: more than 256 groups at every group size, general loop
FILL = 32                 # whole, aligned 1 MiB chunks: waves that take the whole-leaf loop


def _layer():
    rng = np.random.default_rng(20250611)
    lens, big_at = [], None
    for r in range(REPS_BEFORE_BIG + REPS_AFTER_BIG):
        if r == REPS_BEFORE_BIG:
            big_at = len(lens)
            lens.append(BIG)
        lens += PATTERN if r % 2 == 0 else PATTERN[::-1]
        if r == 3:
            lens.append(0)
    first_fill = len(lens)
    lens += [1024 * KIB] * FILL
    offs, pos = [], 0
    for i, l in enumerate(lens):
        if i == big_at:
            pos = ((pos + 15) & ~15) + 5       # not 16-B aligned
        elif i >= first_fill or i % 3 == 0:
            pos = (pos + 15) & ~15
        elif i % 3 == 1:
            pos += 3
        offs.append(pos)
        pos += l
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    ch = np.zeros(len(lens), nydus_gpu.CHUNK_DTYPE)
    ch["offset"], ch["length"] = offs, lens
    ch["file_index"] = np.arange(len(lens))
    return data.tobytes(), ch, big_at


@pytest.fixture(scope="module")
def ref(oracle):
    data, ch, big_at = _layer()
    assert len(data) // KIB + len(ch) > QUAD_MAX_LEAVES     # b3_groups, not the quad kernels
    assert int(ch["length"].max()) <= CHUNK_SIZE and ch["offset"][big_at] % 16 == 5
    leaves = np.maximum(1, (ch["length"].astype(np.int64) + KIB - 1) // KIB)
    assert set(range(1, 18)) <= set(leaves.tolist())
    for D in (1, 2, 3, 4):
        # multi-group chunks take group slots in chunk order, single-group ones come after
        groups = np.where(leaves > (1 << D), (leaves + (1 << D) - 1) >> D, 0)
        base = np.concatenate(([0], np.cumsum(groups)))
        assert groups[big_at] > WINDOW, D
        # the window the big chunk starts in also holds chunks that finish
        # inside it: their trees run in the storage the stacks had
        w = base[big_at] // WINDOW
        assert base[big_at] % WINDOW and any(
            groups[i] > 1 and base[i] // WINDOW == w == (base[i + 1] - 1) // WINDOW
            for i in range(big_at)), D
    dig = oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), "blake3")
    for a in (ch, dig):
        a.setflags(write=False)
    return data, ch, dig


CASES = [(lanes, (lm + 1) << LOAD_MODE_SHIFT) for lanes in (2, 4, 8, 16) for lm in LOAD_MODES] + \
        [(lanes, GRID) for lanes in (2, 4, 8, 16)] + [(1, 0)]


@pytest.mark.parametrize("lanes,flags", CASES, ids=[f"lanes{l}-flags{f:#x}" for l, f in CASES])
def test_lds_stack_vs_oracle(ref, lanes, flags):
    data, ch, dig = ref
    with nydus_gpu.Engine(digester="blake3", chunk_size=CHUNK_SIZE, leaves_per_lane=lanes,
                          flags=flags) as eng:
        out, st = eng.process(data, ch)
    bad = np.nonzero((out["digest"] != dig).any(axis=1))[0]
    assert bad.size == 0, (f"digest: {bad.size} bad chunks, first ids={bad[:8].tolist()} "
                           f"lengths={ch['length'][bad[:8]].tolist()}")
    assert st["chunks"] == len(ch)
