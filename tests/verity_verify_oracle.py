"""Verity verify restated with hashlib: the oracle of the verify tests
(include/nydus_gpu.h, "Verity verify"; csrc/verity.hip).

The inputs are the data, the STORED tree (layout of tests/verity_oracle.py) and
a trusted root.  With first[l] the tree block at which level l starts:
  * data block i is bad iff SHA-256 of its 512 bytes differs from the 32 stored
    bytes at tree offset first[0] * 4096 + 32 i (no tree: from the root);
  * tree block first[l] + j has a bad hash iff SHA-256 of its 4096 stored bytes
    differs from the 32 stored bytes at first[l + 1] * 4096 + 32 j; the top
    block is compared with the root;
  * level l has a bad spare area iff a byte of its last hash block after that
    block's last digest is not zero.
tests/test_verity_verify_oracle.py pins "nothing found" to libcryptsetup's
userspace verification where that library is present."""
import hashlib

import numpy as np

import verity_oracle as vo


def _sha_rows(rows: np.ndarray) -> np.ndarray:
    return np.frombuffer(b"".join(hashlib.sha256(x).digest() for x in rows), np.uint8).reshape(len(rows), 32)


def verdicts_from_leaves(dig, tree, root):
    """verdicts() from the SHA-256 of every data block as it is now ((n, 32)
    uint8), so that a caller with few distinct data blocks hashes each once."""
    dig = np.ascontiguousarray(dig, np.uint8).reshape(-1, 32)
    n = len(dig)
    lay = vo.layout(n * vo.DATA_BLOCK)
    tr = np.frombuffer(tree, np.uint8)
    assert tr.size == lay["tree_bytes"] and len(root) == 32
    if lay["levels"] == 0:
        return ([0] if dig[0].tobytes() != bytes(root) else []), [], []
    first, sizes = lay["first"], lay["level_blocks"]
    stored0 = tr[first[0] * vo.HASH_BLOCK:][:32 * n].reshape(n, 32)
    bad_data = np.flatnonzero((stored0 != dig).any(axis=1)).tolist()
    bad_hash, spare = [], []
    for l in range(lay["levels"]):
        blk = tr[first[l] * vo.HASH_BLOCK:(first[l] + sizes[l]) * vo.HASH_BLOCK].reshape(-1, vo.HASH_BLOCK)
        if l + 1 < lay["levels"]:
            want = tr[first[l + 1] * vo.HASH_BLOCK:][:32 * sizes[l]].reshape(-1, 32)
        else:
            want = np.frombuffer(bytes(root), np.uint8).reshape(1, 32)
        bad_hash += [first[l] + int(j) for j in np.flatnonzero((_sha_rows(blk) != want).any(axis=1))]
        used = (n if l == 0 else sizes[l - 1]) - vo.FANOUT * (sizes[l] - 1)
        if blk[-1, 32 * used:].any():
            spare.append(l)
    return bad_data, sorted(bad_hash), spare


def verdicts(data, tree, root):
    """(bad data blocks, tree blocks with a bad hash, levels with a bad spare
    area), each ascending; all empty iff the image verifies."""
    return verdicts_from_leaves(vo.leaf_digests(data), tree, root)


def level_of(lay: dict, t: int):
    """(level, index in the level) of tree block t, by walking the levels."""
    for l in range(lay["levels"]):
        if lay["first"][l] <= t < lay["first"][l] + lay["level_blocks"][l]:
            return l, t - lay["first"][l]
    raise ValueError(f"tree block {t} of {lay}")


def findings(found, data_blocks: int, hash_offset: int) -> list:
    """The findings list of ngpu_verity_verify_image for verdicts `found`, as
    Engine.verity_verify_image's bad_list holds it: tree findings in tree-block
    order (a block's HASH entry before its SPARE entry), then the data blocks."""
    bad_data, bad_hash, spare = found
    lay = vo.layout(data_blocks * vo.DATA_BLOCK)
    tree = [(t, 0, "HASH") for t in bad_hash]
    tree += [(lay["first"][l] + lay["level_blocks"][l] - 1, 1, "SPARE") for l in spare]
    out = []
    for t, _, reason in sorted(tree):
        l, j = level_of(lay, t)
        span = vo.FANOUT ** (l + 1)
        out.append({"reason": reason, "level": l, "block": t, "first_data_block": j * span,
                    "last_data_block": min(data_blocks, (j + 1) * span) - 1,
                    "file_offset": hash_offset + vo.HASH_BLOCK * t})
    out += [{"reason": "DATA", "level": 0, "block": i, "first_data_block": i, "last_data_block": i,
             "file_offset": vo.DATA_BLOCK * i} for i in bad_data]
    return out


def rehash_up(tree: bytearray, data_blocks: int, level: int, index: int) -> bytes:
    """After a change to block `index` of `level`: its digest into its parent
    slot, and so on up to the top.  Returns the new root."""
    lay = vo.layout(data_blocks * vo.DATA_BLOCK)
    while True:
        at = (lay["first"][level] + index) * vo.HASH_BLOCK
        h = hashlib.sha256(tree[at:at + vo.HASH_BLOCK]).digest()
        if level + 1 == lay["levels"]:
            return h
        slot = lay["first"][level + 1] * vo.HASH_BLOCK + 32 * index
        tree[slot:slot + 32] = h
        level, index = level + 1, index // vo.FANOUT


# ---- single damages, for any image with the kind's precondition -----------------
KINDS = ["data", "level0_digest", "top", "root", "spare", "spare_consistent"]


def applies(kind: str, data_blocks: int) -> bool:
    lay = vo.layout(data_blocks * vo.DATA_BLOCK)
    if kind in ("data", "root"):
        return True
    if kind in ("level0_digest", "top"):
        return lay["levels"] > 0
    return lay["levels"] > 0 and data_blocks % vo.FANOUT != 0  # level 0's last block has a spare area


def damage(kind: str, data: bytes, tree: bytes, root: bytes):
    """(data, tree, root, expected verdicts) after one damage of `kind` to a
    clean image."""
    n = len(data) // vo.DATA_BLOCK
    lay = vo.layout(len(data))
    d, t = bytearray(data), bytearray(tree)
    if kind == "data":
        i = n // 2
        d[i * vo.DATA_BLOCK + 17] ^= 0x40
        return bytes(d), tree, root, ([i], [], [])
    if kind == "root":
        r = bytes([root[0] ^ 1]) + root[1:]
        return data, tree, r, (([0], [], []) if lay["levels"] == 0 else ([], [0], []))
    first, sizes = lay["first"], lay["level_blocks"]
    if kind == "level0_digest":
        j = sizes[0] - 1
        s = (n - 1) % vo.FANOUT  # the last digest of the last block
        t[(first[0] + j) * vo.HASH_BLOCK + 32 * s + 31] ^= 0x01
        return data, bytes(t), root, ([vo.FANOUT * j + s], [first[0] + j], [])
    if kind == "top":
        t[5] ^= 0x80  # digest slot 0 of the top block: the top's own hash, and its first child
        if lay["levels"] == 1:
            return data, bytes(t), root, ([0], [0], [])
        return data, bytes(t), root, ([], [0, first[lay["levels"] - 2]], [])
    last = first[0] + sizes[0] - 1
    t[(last + 1) * vo.HASH_BLOCK - 1] = 1  # the last byte of level 0's spare area
    if kind == "spare":
        return data, bytes(t), root, ([], [last], [0])
    assert kind == "spare_consistent"
    r = rehash_up(t, n, 0, sizes[0] - 1)
    return data, bytes(t), r, ([], [], [0])
