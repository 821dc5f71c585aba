"""The layers of the SHA-256 matrix select the kernels the matrix is about, and
put every padding edge at every lane position.

CPU only: the conditions under which test_gpu_sha_matrix.py runs all seven
kernels of csrc/sha256.hip (sha256_split, sha256_lane, sha256_pair<1,U>,
<1,M>, <2,U>, <2,M>, <4,M>) on ragged waves, the Python mirror of the selection
rule against the header's own picks (tests/cpp/sha256_plan_test.cpp with
arguments), and hashlib against the CPU oracle."""
import subprocess

import numpy as np
import pytest

import nydus_gpu

import sha_shapes as ss


@pytest.fixture(scope="module")
def forms():
    """(layer, pad) -> (data, chunks), built once."""
    out = {("C", False): ss.layer_c(False)}
    for name, fn in (("E", ss.layer_e), ("R", ss.layer_r)):
        for pad in (True, False):
            out[(name, pad)] = fn(pad)
    return out


def _inside(data, ch, chunk_size):
    assert ch.dtype == nydus_gpu.CHUNK_DTYPE
    off, ln = ch["offset"].astype(np.int64), ch["length"].astype(np.int64)
    assert (ln >= 1).all() and (ln <= chunk_size).all()  # the host path refuses longer ones
    assert (off[1:] >= (off + ln)[:-1]).all()            # in order, no overlap
    assert off[-1] + ln[-1] == len(data)                 # the last chunk ends with the buffer


def _classes(ch):
    off, ln = ch["offset"].astype(np.int64), ch["length"].astype(np.int64)
    tail = np.array([ss.tail_class(l) for l in ln])
    align = np.where(off % 16 == 0, "A", np.where(off % 2 == 1, "O", "-"))
    return tail, align


@pytest.mark.parametrize("name", ["E", "R"])
def test_padded_and_plain_forms_hold_the_same_chunks(forms, name):
    (dp, cp), (du, cu) = forms[(name, True)], forms[(name, False)]
    chunk_size = ss.LAYERS[name][1]
    _inside(dp, cp, chunk_size)
    _inside(du, cu, chunk_size)
    n = len(cp)
    assert n == len(cu) == {"E": ss.E_CHUNKS, "R": ss.R_CHUNKS}[name]
    assert np.array_equal(cp["length"], cu["length"])
    shift = cp["offset"].astype(np.int64) - cu["offset"].astype(np.int64)
    first = n - 32
    assert (shift[:first] == 0).all() and (shift[first:] == shift[-1]).all()  # one gap, before the last group
    assert shift[-1] > 0 and shift[-1] % 16 == 0
    for i in range(n):
        o, p, l = int(cu["offset"][i]), int(cp["offset"][i]), int(cu["length"][i])
        assert du[o:o + l] == dp[p:p + l], i
    assert not ss.sha_mixed(n, len(dp), chunk_size)
    assert ss.sha_mixed(n, len(du), chunk_size)
    assert len(dp) >= {"E": 3686400, "R": 13762560}[name] == n * chunk_size // 16 * 15
    assert len(dp) < n * chunk_size // 16 * 15 + 16  # and no larger than it has to be


@pytest.mark.parametrize("pad", [True, False])
def test_layer_e_edges_at_every_position(forms, pad):
    data, ch = forms[("E", pad)]
    ln = ch["length"].astype(np.int64)
    assert sorted(set(ln.tolist())) == list(range(1, 321))    # every length 1..320
    nb = ss.blocks_of(ln)
    assert sorted(set(nb.tolist())) == [1, 2, 3, 4, 5, 6]
    two_block_tails = {int(l) for l in ln if ss.tail_class(l) == "T2"}
    assert len(two_block_tails) == 40
    assert {int(l) for l in ln if l % 64 == 0} == {64, 128, 192, 256, 320}
    tail, align = _classes(ch)
    assert (align != "-").all()
    pos = np.arange(len(ch)) % 32
    for p in range(32):
        at = pos == p
        seen = set(zip(tail[at].tolist(), align[at].tolist()))
        assert seen == {(t, a) for t in ("T1", "T2", "Z") for a in ("A", "O")}, (p, seen)
        assert set((nb[at] % 2).tolist()) == {0, 1}, p       # both halves of the schedule wave
    for g in range(len(ch) // 32):
        assert len(set(nb[32 * g:32 * g + 32].tolist())) >= 2, g  # no wave of any kernel is uniform
    # 960 = 7.5 x 128: the last pair<4> workgroup has two groups past n
    pick = ss.sha_pick(5, len(ch), False)
    assert pick["name"] == "pair<4,M>" and pick["grid"] == 8
    assert (pick["grid"] * pick["chunks_per_wg"] - len(ch)) // 32 == 2
    # split and pair<2> end on a whole workgroup, lane in the middle of one
    assert len(ch) % 64 == 0 and len(ch) % 256 == 192


@pytest.mark.parametrize("pad", [True, False])
def test_layer_r_groups(forms, pad):
    data, ch = forms[("R", pad)]
    off, ln = ch["offset"].astype(np.int64), ch["length"].astype(np.int64)
    nb = ss.blocks_of(ln)
    g = [slice(32 * k, 32 * k + 32) for k in range(7)]
    assert (ln[g[0]] == 65536).all() and (off[g[0]] % 16 == 0).all()
    assert ln[g[1]][13] == 65536
    rest = np.delete(ln[g[1]], 13)
    assert (rest >= 1).all() and (rest <= 200).all()
    assert (ln[g[2]] <= 55).all() and (nb[g[2]] == 1).all()
    assert (off[g[3]] % 2 == 1).all() and len(set(nb[g[3]].tolist())) >= 16
    assert (np.diff(nb[g[4]]) < 0).all()                      # strictly descending block counts
    for p in range(32):
        if p in ss.R_G5_LONG_AT:
            assert nb[g[5]][p] >= 300, p
        else:
            assert nb[g[5]][p] <= 4, p
    assert ss.R_G5_LONG_AT == (7, 8, 31)
    assert (off[g[6]] % 16 == 0).all() and len(set(nb[g[6]].tolist())) >= 16
    assert nb.max() == 1025                                    # the longest chain
    # pair<4>: workgroup 0 shares s_nbmax between two full groups, an all-one-block
    # group and a ragged one; workgroup 1 holds three groups and an absent one
    pick = ss.sha_pick(5, len(ch), False)
    assert pick["chunks_per_wg"] == 128 and pick["grid"] == 2
    maxes = [int(nb[g[k]].max()) for k in range(7)]
    assert maxes[:3] == [1025, 1025, 1] and maxes[3] > 1
    assert len(ch) - 128 == 3 * 32
    # the prefixes are mixed through n % 32
    for n in ss.R_PREFIXES:
        assert n % 32 != 0 and ss.sha_mixed(n, 1 << 40, ss.R_CHUNK_SIZE)


def test_layer_c_counts_and_auto_picks(forms):
    data, ch = forms[("C", False)]
    _inside(data, ch, ss.C_CHUNK_SIZE)
    ln = ch["length"].astype(np.int64)
    assert len(ch) == 32769 and ln.min() == 1 and ln.max() == 200
    assert (ch["offset"][1:] == (ch["offset"] + ch["length"])[:-1]).all()  # back to back
    assert 3_200_000 <= len(data) <= 3_400_000
    names = [ss.pick_name(0, n, len(data), ss.C_CHUNK_SIZE) for n in ss.C_PREFIXES]
    assert names == ["pair<2,U>", "pair<4,M>", "pair<4,M>", "lane"]
    assert all(ss.sha_mixed(n, len(data), ss.C_CHUNK_SIZE) for n in ss.C_PREFIXES)
    with pytest.raises(ValueError):
        ss.layer_c(True)
    # n = 32769: a last partial workgroup in every kernel
    for per in (32, 64, 128, 256):
        assert len(ch) % per == 1


def test_all_seven_kernels_are_selected(forms):
    """By the calls of test_every_kernel_vs_hashlib alone (layers E and R, whole),
    so every kernel runs on ragged waves, pair<1,M> and pair<2,M> included."""
    ran = {}
    for layer, pad, n, flags in ss.matrix_calls():
        data, ch = forms[(layer, pad)]
        if layer in "ER" and n == len(ch):
            ran.setdefault(ss.pick_name(flags, n, len(data), ss.LAYERS[layer][1]), []).append((layer, pad, flags))
    assert sorted(ran) == sorted(ss.KERNELS), ran
    for layer in "ER":
        for k in ("pair<1,M>", "pair<2,M>"):
            assert any(c[0] == layer and c[1] for c in ran[k]), (layer, k)
        for k in ("pair<1,U>", "pair<2,U>"):
            assert any(c[0] == layer and not c[1] for c in ran[k]), (layer, k)


def test_mirror_equals_the_header(forms, tmp_path):
    """Every (layer, form, prefix, variant) of the GPU matrix, and the sizes at
    which the rule steps, through the header's own sha_mixed and sha_pick."""
    exe = ss.build_plan_test(str(tmp_path / "sha256_plan_test"))
    quads = []
    for layer, pad, n, flags in ss.matrix_calls():
        data, _ = forms[(layer, pad)]
        quads.append((ss.variant_of(flags), n, len(data), ss.LAYERS[layer][1]))
    for v in (-1, 0, 1, 2, 3, 4, 5, 6):
        for n in (1, 31, 32, 33, 16384, 16385, 32768, 32769):
            for cs in (0x1000, 0x1000000):
                thr = n * cs // 16 * 15
                quads += [(v, n, thr - 1, cs), (v, n, thr, cs)]
    quads = sorted(set(quads))
    args = [str(x) for q in quads for x in q]
    out = subprocess.check_output([exe] + args, text=True, timeout=120).splitlines()
    assert out[-1] == "ok" and len(out) == len(quads) + 1
    names = set()
    for (v, n, length, cs), line in zip(quads, out):
        f = line.split()
        mixed = ss.sha_mixed(n, length, cs)
        p = ss.sha_pick(v, n, mixed)
        assert f == ["pick", str(v), str(n), str(length), str(cs), str(int(mixed)), p["name"],
                     str(p["chunks_per_wg"]), str(p["threads"]), str(p["grid"])], line
        names.add(p["name"])
    assert names == set(ss.KERNELS)
    assert [ss.variant_of(f) for f in ss.VARIANT_FLAGS] == [-1, 0, 1, 2, 4, 5]


def test_builders_are_deterministic(forms):
    for (layer, pad), (data, ch) in forms.items():
        d2, c2 = ss.LAYERS[layer][0](pad)
        assert d2 == data and c2.tobytes() == ch.tobytes(), (layer, pad)


def test_hashlib_equals_the_oracle_and_duplicates_are_planted(forms, oracle):
    for (layer, pad), (data, ch) in forms.items():
        dig = ss.hashlib_digests(data, ch)
        assert np.array_equal(dig, oracle.digest_chunks(data, ch.view(oracle.CHUNK_DTYPE), "sha256")), (layer, pad)
        dec, _ = oracle.dedup(dig, ch["length"])
        long_intra = (dec["kind"] == nydus_gpu.INTRA) & (ch["length"] > 8)
        assert long_intra.sum() >= 4, (layer, pad)  # not the chance repeats of 1-byte chunks
    for layer in "ER":  # the same digests in both forms
        a = ss.hashlib_digests(*forms[(layer, True)])
        assert np.array_equal(a, ss.hashlib_digests(*forms[(layer, False)]))
