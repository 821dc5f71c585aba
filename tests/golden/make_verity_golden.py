#!/usr/bin/env python3
"""Writes tests/golden/verity.json: the known answers of the dm-verity tree for
data `byte i = i % 251` at 1, 129 and 16385 data blocks (0, 2 and 3 levels),
from the hashlib restatement in tests/verity_oracle.py.  The same values came
out of libcryptsetup (crypt_format "VERITY", sha256, format 1, 512 / 4096-byte
blocks, no header, empty salt) when the file was first written;
tests/test_verity_oracle.py repeats that comparison where the library exists.

  python tests/golden/make_verity_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import verity_oracle  # noqa: E402


def main():
    rows = []
    for n in (1, 129, 16385):
        data = verity_oracle.pattern(n)
        lay = verity_oracle.layout(len(data))
        tree, root = verity_oracle.tree(data)
        rows.append({"data_blocks": n, "levels": lay["levels"], "hash_offset": lay["hash_offset"],
                     "tree_bytes": lay["tree_bytes"], "root": root.hex(),
                     "tree_sha256": hashlib.sha256(tree).hexdigest() if tree else None})
    with open(os.path.join(HERE, "verity.json"), "w") as f:
        json.dump({"pattern": "byte i = i % 251", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
