"""The hash rules of the chunk dict (csrc/dict_hash.hpp: digest_tag,
digest_bucket, owner_of) on the CPU, through tests/cpp/dict_hash_test.cpp
(g++ with ASan/UBSan; no GPU).

  owners   the header's two forms, dist.owner_of, dedup_cases.owner_of and the
           ABI's formula agree on every 16-bit prefix for every W in 1..64
  mirror   dedup_cases.home_slot / tag_of -- what every crafted-digest test
           builds its chains with -- equal the header on a fixed digest list
  chains   a node part's table (rows of one owner only) reads no more slots
           per probe than a table of unconstrained digests: each mean
           <= 1.10 x the W = 1 run of the same program.  (The low k bits of
           `bucket words x odd constant` depend on the low k bits of the words,
           i.e. on the digest bytes the owner rule partitions on: without the
           fold in digest_bucket a part's rows home on 256 / W of the 256 slot
           residues.  Seed-to-seed spread of the means is about 1 %; the
           unfolded product gives 1.20x at W = 2 and 2.3x at W = 8.)
"""
import os
import subprocess

import numpy as np
import pytest

import dedup_cases as dc
from conftest import ROOT

# prefixes hi at which (hi * W) >> 16 steps: ceil(k * 65536 / W), k = 1..W-1
BOUNDARIES = {3: [21846, 43691],
              5: [13108, 26215, 39322, 52429],
              7: [9363, 18725, 28087, 37450, 46812, 56174]}
CHAIN_OWNERS = [(2, 1), (3, 1), (8, 3), (64, 17)]
CHAIN_BOUND = 1.10


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dict_hash") / "dict_hash_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "dict_hash_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=300)
    lines = out.splitlines()
    assert lines[-1] == "ok", out[-2000:]
    return [l.split() for l in lines[:-1]]


def test_owner_rule_agreement(report):
    import torch
    from nydus_gpu.dist import owner_of
    steps = {int(l[1]): [int(x) for x in l[2:]] for l in report if l[0] == "owners"}
    assert sorted(steps) == list(range(1, 65))
    hi = np.arange(65536, dtype=np.int64)
    d = np.zeros((65536, 32), np.uint8)
    d[:, 0], d[:, 1] = hi >> 8, hi & 0xFF
    d[:, 2:] = np.random.default_rng(5).integers(0, 256, (65536, 30), dtype=np.uint8)
    t = torch.from_numpy(d)
    for W in range(1, 65):
        formula = (hi * W) >> 16
        assert np.array_equal(owner_of(t, W).numpy(), formula), W
        assert np.array_equal(dc.owner_of(d, W), formula), W
        # the program checked its two forms against the formula on every prefix
        # and printed where the owner steps: a monotone function from 0 is its steps
        assert steps[W] == (np.flatnonzero(np.diff(formula)) + 1).tolist(), W
        assert formula[0] == 0 and formula[-1] == W - 1
    for W, bounds in BOUNDARIES.items():
        assert steps[W] == bounds
        for k, b in enumerate(bounds):
            assert (b * W) >> 16 == k + 1 and ((b - 1) * W) >> 16 == k


def test_python_mirror_equals_the_header(report):
    rows = [l for l in report if l[0] == "digest"]
    assert len(rows) == 48
    d = np.stack([np.frombuffer(bytes.fromhex(l[1]), np.uint8) for l in rows])
    assert len({bytes(x) for x in d}) == len(d)
    tags = np.array([int(l[2]) for l in rows], np.uint32)
    assert np.array_equal(dc.tag_of(d), tags)
    raw = np.ascontiguousarray(d[:, 8:12]).view("<u4")[:, 0]
    assert (raw == 0xFFFFFFFF).sum() >= 5 and (tags[raw == 0xFFFFFFFF] == 0xFFFFFFFE).all()
    assert (raw == 0xFFFFFFFE).sum() >= 5 and (tags != 0xFFFFFFFF).all()
    for col, mask in ((3, 63), (4, 1023), (5, (1 << 17) - 1)):
        want = np.array([int(l[col]) for l in rows], np.uint64)
        assert np.array_equal(dc.home_slot(d, mask), want), mask
        assert len(set(want.tolist())) > min(len(rows), mask + 1) // 3  # not a constant column


def test_part_tables_chain_no_longer_than_a_plain_dict(report, capsys):
    chains = {(int(l[1]), int(l[2])): (float(l[3]), float(l[4]), int(l[5])) for l in report if l[0] == "chain"}
    ref_hit, ref_miss, ref_long = chains[(1, 0)]
    with capsys.disabled():
        print(f"\nslots read per probe, 60,000 rows in 131,072 slots: any digest hit {ref_hit:.3f} "
              f"miss {ref_miss:.3f} longest {ref_long}", end="")
        for W, o in CHAIN_OWNERS:
            h, m, lg = chains[(W, o)]
            print(f"; owner {o} of {W} hit {h:.3f} ({h / ref_hit:.3f}x) miss {m:.3f} "
                  f"({m / ref_miss:.3f}x) longest {lg}", end="")
    # the reference itself is what linear probing gives at this load (a = 60000 / 131072):
    # (1 + 1 / (1 - a)) / 2 per hit, (1 + 1 / (1 - a)^2) / 2 per miss (the empty slot counted)
    a = 60000 / 131072
    assert abs(ref_hit - (1 + 1 / (1 - a)) / 2) < 0.03
    assert abs(ref_miss - ((1 + 1 / (1 - a) ** 2) / 2)) < 0.08
    for W, o in CHAIN_OWNERS:
        h, m, _ = chains[(W, o)]
        assert h <= CHAIN_BOUND * ref_hit, (W, o, h, ref_hit)
        assert m <= CHAIN_BOUND * ref_miss, (W, o, m, ref_miss)
