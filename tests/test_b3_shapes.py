"""The layers of the BLAKE3 matrix select the kernels the matrix is about.

CPU only: the conditions under which test_gpu_b3_matrix.py runs every planner,
leaf kernel and branch of b3_groups<D> it claims to (launch_blake3,
csrc/blake3.hip: kSmallPlanChunks = 4096, kQuadMaxLeaves = 40960)."""
import numpy as np
import pytest

import nydus_gpu

import b3_shapes

SMALL_PLAN_CHUNKS = 4096
QUAD_MAX_LEAVES = 40960
KIB = 1024


@pytest.fixture(scope="module")
def layer_a():
    return b3_shapes.layer_a()


@pytest.fixture(scope="module")
def layer_b():
    return b3_shapes.layer_b()


def _inside(data, ch, chunk_size):
    assert ch.dtype == nydus_gpu.CHUNK_DTYPE
    end = ch["offset"].astype(np.int64) + ch["length"]
    assert (end <= len(data)).all()
    assert (ch["length"] >= 1).all() and (ch["length"] <= chunk_size).all()
    # chunks follow each other without overlap (a launch is sized by the buffer)
    assert (ch["offset"][1:].astype(np.int64) >= end[:-1]).all()


def test_layer_a_selects_plan_small_and_groups(layer_a):
    data, ch = layer_a
    n = len(ch)
    _inside(data, ch, b3_shapes.A_CHUNK_SIZE)
    assert n <= SMALL_PLAN_CHUNKS
    assert len(data) // 1024 + n > QUAD_MAX_LEAVES  # D = 0: b3_plan_small + b3_groups<0>
    for D in range(5):
        single, inwin, straddle = b3_shapes.plan_counts(ch, D)
        print(f"A D={D}: single-group {single}, in-window {inwin}, straddling {straddle}")
        assert single + inwin + straddle == n
        assert single >= 300 and inwin >= 500 and straddle >= 7, (D, single, inwin, straddle)


def test_layer_a_lengths_and_offsets(layer_a):
    data, ch = layer_a
    ln, off = ch["length"].astype(np.int64), ch["offset"].astype(np.int64)
    assert 45 << 20 <= len(data) <= 47 << 20 and 1350 <= len(ch) <= 1450
    for l in b3_shapes.BLOCK_EDGES:
        assert (ln == l).any(), l
    for g in b3_shapes.GROUP_KIB:
        for m in (1, 2, 3):
            for d in (-1, 0, 1):
                at = off[ln == m * g * KIB + d]
                assert (at % 16 == 0).any() and (at % 2 == 1).any(), (g, m, d)
    big = off[ln == 1025 * KIB + 1]
    assert len(big) == 1 and big[0] % 16 == 0
    wide = off[ln == 257 * 16 * KIB + 1]
    assert len(wide) == 1 and wide[0] % 2 == 1
    # the closing run: whole aligned 64 KiB chunks (waves of the fast path), then
    # the chunk whose tail block ends with the buffer
    run = slice(len(ch) - 1 - b3_shapes.A_RUN, len(ch) - 1)
    assert (ln[run] == 64 * KIB).all() and (off[run] % 16 == 0).all()
    assert ln[-1] == 37 * KIB + 5 and off[-1] % 16 == 0
    assert off[-1] + ln[-1] == len(data)
    # both alignments among the ragged chunks
    body = off[:run.start]
    assert (body % 16 == 0).sum() >= 300 and (body % 2 == 1).sum() >= 300


def test_layer_b_selects_grid_plan_and_quad_leaves(layer_b):
    data, ch = layer_b
    n = len(ch)
    _inside(data, ch, b3_shapes.B_CHUNK_SIZE)
    assert n == 4500 and SMALL_PLAN_CHUNKS < n
    assert len(data) // 1024 + n <= QUAD_MAX_LEAVES  # D = 0: grid plan + b3_quad_leaves
    assert 16 << 20 <= len(data) <= 19 << 20
    assert (ch["offset"][0::2] % 16 == 0).all()
    for D in range(5):
        single, inwin, straddle = b3_shapes.plan_counts(ch, D)
        print(f"B D={D}: single-group {single}, in-window {inwin}, straddling {straddle}")
        assert single + inwin + straddle == n
        assert single >= 1000 and inwin >= 200 and straddle >= 2, (D, single, inwin, straddle)


def test_builders_are_deterministic(layer_a, layer_b):
    for fn, (data, ch) in ((b3_shapes.layer_a, layer_a), (b3_shapes.layer_b, layer_b)):
        d2, c2 = fn()
        assert d2 == data and c2.tobytes() == ch.tobytes()


def test_plan_counts_by_hand():
    ch = np.zeros(4, nydus_gpu.CHUNK_DTYPE)
    # D = 1: 2 leaves (single); 255 groups at base 0 (in window); 2 groups at
    # base 255 (straddles 255 | 256); 3 groups at base 257 (in window)
    ch["length"] = [2048, 2 * 255 * 1024, 2049, 5 * 1024]
    assert b3_shapes.plan_counts(ch, 1) == (1, 2, 1)
    # D = 0: groups 2, 510, 3, 5 at bases 0, 2, 512, 515: the second straddles
    assert b3_shapes.plan_counts(ch, 0) == (0, 3, 1)
    assert b3_shapes.plan_counts(ch, 4) == (3, 1, 0)
