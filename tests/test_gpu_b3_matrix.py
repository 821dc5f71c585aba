"""The BLAKE3 digest stage's whole dispatch matrix on ragged chunks, bit-exact
against the CPU oracle: every load mode of b3_groups<D, LM> x every leaf-group
size x both planners (launch_blake3, csrc/blake3.hip), the natural grid plan
of a layer of more than 4,096 chunks, and the narrow b3_tree over more than
one tile.  The layers and the CPU proof of which kernels they select are in
b3_shapes.py / test_b3_shapes.py.  Run on a gfx950 box: pytest -m gpu."""
import numpy as np
import pytest

import nydus_gpu

import b3_shapes

pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16]
LOAD_MODES = [0, 1, 2, 3, 5]   # the modes the library has a kernel for
LOAD_MODE_SHIFT = 8            # NGPU_FLAG_LOAD_MODE_SHIFT: bits 8..10 = 1 + load mode
GRID = nydus_gpu.FLAG_GRID_STAGES
DEDUP_FIELDS = ("kind", "index", "ref", "uncompressed_offset")


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(chunk_size, lanes, flags):
        k = (chunk_size, lanes, flags)
        if k not in cache:
            cache[k] = nydus_gpu.Engine(digester="blake3", chunk_size=chunk_size,
                                        leaves_per_lane=lanes, flags=flags)
        return cache[k]
    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def refs(oracle):
    """Per layer: the bytes, the chunks, the engine chunk size and the oracle's
    digests and dedup decisions, computed once and only read by the tests."""
    out = {}
    for name, build, chunk_size in (("A", b3_shapes.layer_a, b3_shapes.A_CHUNK_SIZE),
                                    ("B", b3_shapes.layer_b, b3_shapes.B_CHUNK_SIZE)):
        data, ch = build()
        dig = oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), "blake3")
        dec, _ = oracle.dedup(dig, ch["length"])
        assert (dec["kind"] == nydus_gpu.INTRA).sum() >= 10  # the planted duplicates
        for a in (ch, dig, dec):
            a.setflags(write=False)
        out[name] = (data, ch, chunk_size, dig, dec)
    return out


def _where(ch, bad):
    ids = [int(i) for i in bad[:8]]
    return (f"{len(bad)} bad chunks, first ids={ids} lengths={[int(ch['length'][i]) for i in ids]} "
            f"offset%16={[int(ch['offset'][i]) % 16 for i in ids]}")


@pytest.mark.parametrize("lm", LOAD_MODES)
@pytest.mark.parametrize("layer", ["A", "B"])
def test_load_modes_vs_oracle(engines, refs, layer, lm):
    """Load mode lm (sent as flag value lm + 1; 1 << 8 is the explicit default)
    at 1, 2, 4, 8 and 16 leaves per lane under the fused and the grid planner:
    the prefetch cursor across the leaves of a group, the non-temporal and the
    masked partial-block loads, the general loop on whole aligned leaves
    (mode 5), the in-lane merge stack, the lane-balance permutation, the
    in-window trees and the chunks that straddle a window and go to b3_tree."""
    data, ch, chunk_size, dig, dec = refs[layer]
    for lanes in LANES:
        for flags in ((lm + 1) << LOAD_MODE_SHIFT, ((lm + 1) << LOAD_MODE_SHIFT) | GRID):
            out, st = engines(chunk_size, lanes, flags).process(data, ch)
            tag = f"layer {layer} lm={lm} lanes={lanes} flags={flags:#x}"
            bad = np.nonzero((out["digest"] != dig).any(axis=1))[0]
            assert bad.size == 0, f"{tag}: digest: {_where(ch, bad)}"
            for f in DEDUP_FIELDS:
                bad = np.nonzero(out[f] != dec[f])[0]
                assert bad.size == 0, f"{tag}: {f}: {_where(ch, bad)}"
            assert st["chunks"] == len(ch), tag


def test_group_log2_is_what_was_asked(refs):
    """leaves_per_lane reaches the plan: a silently ignored value would run the
    matrix five times at one group size."""
    data, ch, chunk_size, dig, _ = refs["B"]
    for lanes, D in [(0, 0), (1, 0), (2, 1), (4, 2), (8, 3), (16, 4)]:
        with nydus_gpu.Engine(chunk_size=chunk_size, leaves_per_lane=lanes, timing=True) as eng:
            out, _ = eng.process(data, ch)
            assert eng.last_timing()["group_log2"] == D, lanes
        assert np.array_equal(out["digest"], dig), lanes


def test_load_mode_values_the_library_has_no_kernel_for():
    """Flag values 5 and 7 (mode 4, diagnostic builds only, and mode 6) are
    rejected by ngpu_create: the load-mode bits are parsed, not dropped."""
    for v in (5, 7):
        with pytest.raises(nydus_gpu.NgpuError) as ei:
            nydus_gpu.Engine(flags=v << LOAD_MODE_SHIFT)
        assert ei.value.code == nydus_gpu.EINVAL, v
    nydus_gpu.Engine(flags=6 << LOAD_MODE_SHIFT).close()  # mode 5


def test_narrow_tree_more_than_one_tile(oracle):
    """b3_tree<256, 512> over 769 group CVs.  The narrow tree is launched when
    chunk_size / 4 KiB fits its 512-CV tile; only the host path can hold a
    chunk to chunk_size, so descriptors from the device may carry more: the
    tree must then walk several tiles, as the wide one does."""
    import torch
    chunk_size = 0x100000
    rng = np.random.default_rng(769)
    lens = [int(l) for l in rng.integers(1, 4097, 600)]
    lens.insert(300, 3 * (1 << 20) + 1)
    ch = np.zeros(len(lens), nydus_gpu.CHUNK_DTYPE)
    ch["length"] = lens
    ch["offset"] = np.cumsum(lens) - lens
    data = rng.integers(0, 256, int(np.sum(lens)), dtype=np.uint8)
    n = len(ch)
    # the planned path (b3_quad_planned: groups of 4 leaves) with the narrow tree
    assert 512 <= n <= 4096 and len(data) // 1024 + n <= 40960
    assert chunk_size // 4096 <= 512 < (int(ch["length"].max()) + 4095) // 4096 == 769
    dig = oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), "blake3")
    d_data = torch.from_numpy(data).cuda()
    d_ch = torch.from_numpy(ch.view(np.uint8).copy()).cuda()
    for flags in (0, GRID):  # GRID: b3_groups<0> and the wide tree on the same input
        d_out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with nydus_gpu.Engine(chunk_size=chunk_size, flags=flags) as eng:
            st = eng.process_device(d_data.data_ptr(), d_data.numel(), d_ch.data_ptr(), n,
                                    d_out.data_ptr(), want_stats=True)
        out = d_out.cpu().numpy().view(nydus_gpu.RESULT_DTYPE)
        bad = np.nonzero((out["digest"] != dig).any(axis=1))[0]
        assert bad.size == 0, f"flags={flags:#x}: {_where(ch, bad)}"
        assert st["chunks"] == n
