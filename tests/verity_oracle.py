"""The dm-verity hash tree restated with hashlib: the oracle of the Verity tests
(include/nydus_gpu.h, "Verity"; csrc/verity.hip).

Format 1, no superblock, empty salt, sha256, 512-byte data blocks, 4096-byte
hash blocks, as cryptsetup writes and the kernel's dm-verity reads them:
a digest is SHA-256 of a whole data block or a whole hash block; a hash block
is up to 128 consecutive digests of the level below, zero padded; the tree
holds the top level first and level 0 (the one above the data) last; the root
is the digest of the single top hash block, or of the one data block when
there is no tree.  tests/test_verity_oracle.py checks this file against
libcryptsetup where that library is present."""
import hashlib

import numpy as np

DATA_BLOCK, HASH_BLOCK, FANOUT = 512, 4096, 128


def layout(data_bytes: int) -> dict:
    """level_blocks[i] / first[i]: hash blocks of level i (0 = above the data)
    and the tree block at which the level starts."""
    if data_bytes <= 0 or data_bytes % DATA_BLOCK:
        raise ValueError(f"{data_bytes} bytes: not a non-zero multiple of {DATA_BLOCK}")
    n = data_bytes // DATA_BLOCK
    levels = 0
    while (n - 1) >> (7 * levels):
        levels += 1
    sizes, m = [], n
    for _ in range(levels):
        m = -(-m // FANOUT)
        sizes.append(m)
    return {"data_blocks": n, "levels": levels, "level_blocks": sizes,
            "first": [sum(sizes[i + 1:]) for i in range(levels)],
            "hash_offset": -(-data_bytes // HASH_BLOCK) * HASH_BLOCK,
            "tree_bytes": HASH_BLOCK * sum(sizes)}


def leaf_digests(data) -> np.ndarray:
    """(data blocks, 32): SHA-256 of every 512-byte block."""
    b = np.frombuffer(data, np.uint8).reshape(-1, DATA_BLOCK)
    return np.frombuffer(b"".join(hashlib.sha256(x).digest() for x in b), np.uint8).reshape(-1, 32)


def tree_from_leaves(dig: np.ndarray):
    """(tree bytes, root bytes) from the data blocks' digests, so that a caller
    with few distinct data blocks hashes each once."""
    lay = layout(len(dig) * DATA_BLOCK)
    levels, cur = [], np.ascontiguousarray(dig, np.uint8).reshape(-1, 32)
    for m in lay["level_blocks"]:
        blk = np.zeros((m, HASH_BLOCK), np.uint8)
        blk.reshape(-1)[:cur.size] = cur.reshape(-1)
        levels.append(blk)
        cur = np.frombuffer(b"".join(hashlib.sha256(x).digest() for x in blk), np.uint8).reshape(m, 32)
    assert len(cur) == 1
    return b"".join(x.tobytes() for x in reversed(levels)), cur[0].tobytes()


def tree(data):
    """(tree bytes, root bytes) of a block image."""
    return tree_from_leaves(leaf_digests(data))


def image_file(data) -> bytes:
    """What `export --block --verity` leaves: the data, zeros up to the hash
    offset, the tree."""
    data = bytes(data)
    return data + bytes(layout(len(data))["hash_offset"] - len(data)) + tree(data)[0]


def pattern(n_blocks: int) -> bytes:
    """byte i = i % 251, the known-answer input of tests/golden/verity.json."""
    return (np.arange(n_blocks * DATA_BLOCK, dtype=np.int64) % 251).astype(np.uint8).tobytes()
