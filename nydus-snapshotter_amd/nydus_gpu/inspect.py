"""Canonical chunk-table dump of a RAFS v5 / v6 bootstrap or a nydus blob stream —
the comparison form SURVEY.md §8(f) next-2 asks for in place of
`nydus-image inspect` (unavailable here; the reference reads blob ids the same
way, `nydus-image inspect -R blobs`, pkg/tarfs/tarfs.go:284-306).

Chunk tables are written in hash-map iteration order by nydus-image, so two
converters' tables can only be compared as sets keyed by digest: records are
emitted sorted by (digest, blob id, index) with the blob index replaced by the
blob id.

A v5 bootstrap has no chunk table: its records are the chunk infos of every
file's inode, one per distinct (digest, blob, index).  `--tree` dumps the inode
tree instead (ngpu_rafs_dump: every inode depth first with its metadata and
chunk records), and `--diff --tree` compares two trees path by path.

usage:
  python -m nydus_gpu.inspect FILE            # JSON dump of the chunk set
  python -m nydus_gpu.inspect --tree FILE     # JSON dump of the inode tree
  python -m nydus_gpu.inspect --diff A B      # exit 0 iff the chunk sets match
  python -m nydus_gpu.inspect --diff --tree A B  # exit 0 iff the trees match
  python -m nydus_gpu.inspect --check STREAM [--dict BOOTSTRAP]... [--retire BLOBID]... [--distill [N]] [--merge-blob-ids] [--chunk-size N] [--digester D]
                                              # re-digest STREAM's chunks on the GPU; exit 1 if any is bad
  python -m nydus_gpu.inspect --dict BOOTSTRAP [--dict BOOTSTRAP]... [--retire BLOBID]... [--distill [N]] [--merge-blob-ids] --save-dict OUT
                                              # fold the dict bootstraps on the GPU and write the result to OUT
  python -m nydus_gpu.inspect --verity IMAGE [--append]
                                              # the dm-verity tree of a block image; prints its options line
  python -m nydus_gpu.inspect --verity-verify IMAGE --data-blocks N --hash-offset OFF ROOT
                                              # recompute the tree; exit 1 naming the first hash block that differs
  python -m nydus_gpu.inspect --verity-scan IMAGE (--data-blocks N --hash-offset OFF ROOT | --label N,OFF,sha256:ROOT)
                                              # every block against the STORED tree; JSON report, exit 1 on findings
FILE may be a bootstrap (image.boot) or a whole Pack output stream.

`--check` (Engine.check, ngpu_check_stream) needs a GPU: every chunk record of
the stream's image.boot is read from its image.blob, inflated, hashed on the GPU
and compared with the record's digest; records of other blobs must resolve in
the `--dict` chunk-dict bootstrap (without one they are counted as skipped).
Several `--dict` are folded into one dict in the order given (the first is
opened, each further one appended with ChunkDict.extend_bootstrap), as a
conversion run folds each converted image into its chunk dict.
Every `--retire BLOBID` (64 hex characters, or an inner blob index) then drops
that blob's records from the folded dict (ChunkDict.retire), as a registry's
garbage collection does: DICT records of a retired blob no longer resolve.
`--distill [N]` (default 1; ChunkDict.distill, ngpu_dict_distill) then keeps one
row per digest, the first, and only the digests that at least N rows held: a
dict folded from converted layers repeats every chunk a layer reused, and those
rows can never answer.  Blobs left without a row leave; `--merge-blob-ids` also
maps blobs whose table rows repeat a blob id to the first of them (it implies
`--distill`).  The report gains "distill": the info fields.
The digester, chunk size and RAFS version default to the stream's own; the
report is printed as JSON.

`--save-dict OUT` (ChunkDict.save, ngpu_dict_save) needs a GPU: the dict folded
from the `--dict` files, after any `--retire` and `--distill`, is written to OUT as a RAFS v6 dict
bootstrap that `--dict`, ngpu_dict_open and Merge read.  With `--check` the
report gains "saved_dict": {path, entries, blobs, bytes}; without it the command
stands alone, takes chunk size and digester from the first `--dict` bootstrap
unless given, and prints that object.

`--verity` (Engine.verity_file, ngpu_verity_image) needs a GPU: IMAGE is a block
image (`nydus-image export --block`, a multiple of 512 bytes); the line printed
is the one `export --block --verity` prints and pkg/tarfs/tarfs.go:548 parses,
and `--append` leaves the file that command leaves (zeros up to the hash
offset, then the tree).  `--verity-verify` hashes the first N 512-byte blocks
of IMAGE again and compares the root with ROOT and the tree with the bytes at
OFF, on the host.

`--verity-scan` (Engine.verity_verify_file, ngpu_verity_verify_image) needs a
GPU: the stored tree is read as it is and every data block and every stored
hash block is checked against its stored parent digest (the top block against
ROOT), as the kernel's dm-verity would on reading it; the spare area of each
level's last hash block must be zero.  The report is printed as JSON with a
`bad_list` that names each bad data block, and each bad tree block with its
level and the data blocks it covers.  Exit 0: clean; 1: findings; 2: usage or
I/O error.
"""
from __future__ import annotations

import argparse
import json
import struct
import sys

import numpy as np

from . import rafs
from ._lib import NgpuError, rafs_dump, unpack_entry


def bootstrap_bytes(data: bytes) -> bytes:
    """A bootstrap as is, or the image.boot entry of a nydus blob stream."""
    try:
        rafs.detect_fs_version(data)
        return data
    except ValueError:
        pass
    try:
        return unpack_entry(data, "image.boot")[0]
    except NgpuError as e:
        raise ValueError(f"neither a RAFS bootstrap nor a nydus blob stream: {e}") from e


def load_bootstrap(data: bytes) -> dict:
    """{"blob_ids", "chunks" (CHUNK_INFO_DTYPE), "flags", "chunk_size"} of a
    bootstrap or of the image.boot entry of a nydus blob stream."""
    boot = bootstrap_bytes(data)
    if rafs.detect_fs_version(boot) == "v6":
        return rafs.read_v6(boot)
    d = rafs_dump(boot)
    rows = {}
    for ino in d["inodes"]:
        for c in ino.get("chunks", []):
            rows.setdefault((c[0], c[1], c[8]), c)
    recs = np.zeros(len(rows), rafs.CHUNK_INFO_DTYPE)
    for i, c in enumerate(rows.values()):
        recs[i]["block_id"] = np.frombuffer(bytes.fromhex(c[0]), np.uint8)
        (recs[i]["blob_index"], recs[i]["flags"], recs[i]["compressed_offset"], recs[i]["compressed_size"],
         recs[i]["uncompressed_offset"], recs[i]["uncompressed_size"], recs[i]["file_offset"],
         recs[i]["index"]) = c[1:9]
    return {"blob_ids": [b["id"] for b in d["blobs"]], "chunks": recs, "flags": d["flags"],
            "chunk_size": d["chunk_size"]}


def tree(data: bytes) -> dict:
    """The inode tree (ngpu_rafs_dump) with blob indices replaced by blob ids."""
    d = rafs_dump(bootstrap_bytes(data))
    ids = [b["id"] for b in d["blobs"]]
    for ino in d["inodes"]:
        for c in ino.get("chunks", []):
            c[1] = ids[c[1]] if c[1] < len(ids) else f"#{c[1]}"
    return d


def tree_diff(a: dict, b: dict) -> list:
    """Paths missing on one side (-/+) or whose inode differs (~); inode
    numbers aside, as they depend on the tree's numbering, not the content."""
    def key(i):
        return {k: v for k, v in i.items() if k != "ino"}
    pa = {i["path"]: key(i) for i in a["inodes"]}
    pb = {i["path"]: key(i) for i in b["inodes"]}
    out = [("-", p) for p in sorted(pa.keys() - pb.keys())] + [("+", p) for p in sorted(pb.keys() - pa.keys())]
    out += [("~", p) for p in sorted(pa.keys() & pb.keys()) if pa[p] != pb[p]]
    return out


def canonical(b: dict) -> dict:
    ids = b["blob_ids"]
    recs = []
    for r in b["chunks"]:
        bi = int(r["blob_index"])
        recs.append({"digest": bytes(r["block_id"]).hex(),
                     "blob_id": ids[bi] if bi < len(ids) else f"#{bi}",
                     "flags": int(r["flags"]), "compressed_size": int(r["compressed_size"]),
                     "uncompressed_size": int(r["uncompressed_size"]),
                     "compressed_offset": int(r["compressed_offset"]),
                     "uncompressed_offset": int(r["uncompressed_offset"]),
                     "file_offset": int(r["file_offset"]), "index": int(r["index"])})
    recs.sort(key=lambda x: (x["digest"], x["blob_id"], x["index"]))
    return {"flags": int(b["flags"]), "chunk_size": int(b["chunk_size"]),
            "blobs": sorted(set(ids)), "chunks": recs}


def diff(a: dict, b: dict, fields=("digest", "blob_id", "uncompressed_size")) -> list:
    """Records present in one dump and not the other, compared on `fields`."""
    ka = {tuple(r[f] for f in fields) for r in a["chunks"]}
    kb = {tuple(r[f] for f in fields) for r in b["chunks"]}
    return [("-", k) for k in sorted(ka - kb)] + [("+", k) for k in sorted(kb - ka)]


def folded_dict(eng, dict_path=None, retire=None, distill=None, merge_blob_ids=False, report=None):
    """The dict of the --dict bootstraps on `eng`: the first opened, each further
    one appended, then the --retire blobs (ids or inner indices) dropped, then
    (distill: min_refs, or None) distilled, its info into report["distill"].  None
    without a --dict; the caller releases it."""
    paths = [dict_path] if isinstance(dict_path, str) else list(dict_path or [])
    dct = eng.dict_open(paths[0]) if paths else None
    try:
        for p in paths[1:]:
            grown = dct.extend_bootstrap(p)
            dct.release()
            dct = grown
        if retire:
            if dct is None:
                raise ValueError("--retire needs a --dict")
            kept = dct.retire([int(b) if str(b).isdigit() and len(str(b)) < 64 else b for b in retire])
            dct.release()
            dct = kept
        if merge_blob_ids and distill is None:
            distill = 1
        if distill is not None:
            if dct is None:
                raise ValueError("--distill needs a --dict")
            kept, info = dct.distill(distill, merge_blob_ids=merge_blob_ids)
            dct.release()
            dct = kept
            if report is not None:
                report["distill"] = info
        return dct
    except BaseException:
        if dct is not None:
            dct.release()
        raise


def _save(dct, out: str) -> dict:
    if dct is None:
        raise ValueError("--save-dict needs a --dict")
    info = dct.save(out)
    return {"path": out, "entries": info["entries"], "blobs": info["blobs"], "bytes": info["bytes"]}


def save_dict(out: str, dict_path, chunk_size: int = 0, digester: str = None, retire=None, distill=None,
              merge_blob_ids: bool = False) -> dict:
    """The dict folded from the --dict bootstraps (after any --retire and distill)
    written to `out` with ChunkDict.save on GPU 0 -> {path, entries, blobs, bytes},
    and "distill": the info of a distill.  Chunk size and digester default to the
    first bootstrap's."""
    from ._lib import Engine
    paths = [dict_path] if isinstance(dict_path, str) else list(dict_path or [])
    if not paths:
        raise ValueError("--save-dict needs a --dict")
    with open(paths[0], "rb") as f:
        head = f.read(rafs.EXT_OFFSET + 256)
    if rafs.detect_fs_version(head) != "v6":
        raise ValueError(f"{paths[0]}: --save-dict takes RAFS v6 dict bootstraps")
    flags, _, _, cs = struct.unpack_from("<QQII", head, rafs.EXT_OFFSET)
    with Engine(device=0, digester=digester or ("sha256" if flags & 0x8 else "blake3"),
                chunk_size=chunk_size or cs, fs_version=6) as eng:
        extra = {}
        dct = folded_dict(eng, paths, retire, distill, merge_blob_ids, extra)
        try:
            return dict(_save(dct, out), **extra)
        finally:
            dct.release()


def check(path: str, dict_path=None, chunk_size: int = 0, digester: str = None,
          max_bad: int = 64, retire=None, save_dict: str = None, distill=None,
          merge_blob_ids: bool = False) -> dict:
    """Engine.check of the stream in `path` on GPU 0 (the report dict).
    dict_path: a chunk-dict bootstrap, or a list of them folded into one dict;
    retire: blob ids (or inner indices) whose records leave the folded dict first;
    distill: min_refs of a ChunkDict.distill after that (None: none), reported as "distill";
    save_dict: write that dict there (ChunkDict.save), reported as "saved_dict"."""
    from ._lib import Engine
    data = np.fromfile(path, np.uint8)
    boot = bootstrap_bytes(data)
    v6 = rafs.detect_fs_version(boot) == "v6"
    if v6:
        b = rafs.read_v6(boot)
        flags, cs = int(b["flags"]), int(b["chunk_size"])
    else:
        d = rafs_dump(boot)
        flags, cs = int(d["flags"]), int(d["chunk_size"])
    with Engine(device=0, digester=digester or ("sha256" if flags & 0x8 else "blake3"),
                chunk_size=chunk_size or cs, fs_version=6 if v6 else 5) as eng:
        extra = {}
        dct = folded_dict(eng, dict_path, retire, distill, merge_blob_ids, extra)
        try:
            saved = _save(dct, save_dict) if save_dict else None
            rep = eng.check(data, dict=dct, max_bad=max_bad)
            rep.update(extra)
            if saved is not None:
                rep["saved_dict"] = saved
            return rep
        finally:
            if dct is not None:
                dct.release()


def verity(path: str, append: bool = False) -> dict:
    """Engine.verity_file of the block image in `path` on GPU 0 (the info dict)."""
    from ._lib import Engine
    with Engine(device=0) as eng:
        return eng.verity_file(path, append=append)


def verity_verify(path: str, data_blocks: int, hash_offset: int, root: str) -> list:
    """Recompute the tree of the first data_blocks x 512 bytes of `path` on GPU
    0 and compare it with ROOT and with the tree stored at hash_offset.  Returns
    the findings (empty: all equal).  A differing hash block is named at the
    lowest level that has one -- the block closest to the damage: a changed
    data block changes its level-0 hash block and every block above it."""
    from ._lib import Engine, verity_layout
    lay = verity_layout(data_blocks * 512)
    src = np.memmap(path, np.uint8, mode="r")
    if hash_offset < data_blocks * 512 or hash_offset + lay["tree_bytes"] > src.size:
        raise ValueError(f"{path}: {src.size} bytes do not hold {data_blocks} data blocks and a tree of "
                         f"{lay['tree_bytes']} bytes at {hash_offset}")
    with Engine(device=0) as eng:
        tree, info = eng.verity(src[:data_blocks * 512])
    out = []
    if info["root"] != root.lower():
        out.append(f"root differs: computed {info['root']}, expected {root.lower()}")
    stored = src[hash_offset:hash_offset + lay["tree_bytes"]].reshape(-1, 4096)
    bad = np.flatnonzero((tree.reshape(-1, 4096) != stored).any(axis=1))
    if len(bad):
        # level sizes, level 0 first; the tree holds the top level first
        sizes, n = [], data_blocks
        for _ in range(lay["levels"]):
            n = -(-n // 128)
            sizes.append(n)
        first, at = {}, 0
        for lvl in reversed(range(len(sizes))):
            first[lvl] = at
            at += sizes[lvl]
        for lvl in range(len(sizes)):
            b = bad[(bad >= first[lvl]) & (bad < first[lvl] + sizes[lvl])]
            if len(b):
                t = int(b[0])
                j = t - first[lvl]
                span = 128 ** (lvl + 1)
                out.append(f"hash block {t} (level {lvl}, block {j} of the level, file offset "
                           f"{hash_offset + 4096 * t}) differs: it covers data blocks "
                           f"{j * span}..{min(data_blocks, (j + 1) * span) - 1}; "
                           f"{len(bad)} hash block(s) differ in all")
                break
    return out


def verity_scan(path: str, data_blocks: int, hash_offset: int, root: str, max_bad: int = 64) -> dict:
    """Engine.verity_verify_file of `path` on GPU 0 (the report dict): every
    data block and every stored hash block against the stored tree and ROOT."""
    from ._lib import Engine
    with Engine(device=0) as eng:
        return eng.verity_verify_file(path, data_blocks, hash_offset, root, max_bad=max_bad)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m nydus_gpu.inspect")
    ap.add_argument("files", nargs="*")
    ap.add_argument("--check", metavar="STREAM", help="re-digest a Pack output stream's chunks on the GPU")
    ap.add_argument("--dict", metavar="BOOTSTRAP", action="append",
                    help="--check: chunk-dict bootstrap for DICT records (repeat to fold several into one dict)")
    ap.add_argument("--retire", metavar="BLOBID", action="append",
                    help="--check: drop this blob's records from the folded dict first (repeatable)")
    ap.add_argument("--distill", metavar="N", type=lambda x: int(x, 0), nargs="?", const=1, default=None,
                    help="then keep one row per digest, of the digests at least N rows held (default 1)")
    ap.add_argument("--merge-blob-ids", action="store_true",
                    help="--distill: blobs whose table rows repeat a blob id become the first of them")
    ap.add_argument("--save-dict", metavar="OUT",
                    help="write the dict folded from the --dict files (after any --retire) to OUT as a "
                         "RAFS v6 dict bootstrap; with --check the report names it, alone it prints "
                         "{path, entries, blobs, bytes}")
    ap.add_argument("--chunk-size", type=lambda x: int(x, 0), default=0, help="--check: engine chunk size")
    ap.add_argument("--digester", choices=("blake3", "sha256"), help="--check: engine digester")
    ap.add_argument("--verity", metavar="IMAGE", help="dm-verity tree of a block image on the GPU")
    ap.add_argument("--append", action="store_true", help="--verity: append the tree to IMAGE at its hash offset")
    ap.add_argument("--verity-verify", metavar="IMAGE", help="recompute IMAGE's tree and compare (ROOT follows)")
    ap.add_argument("--verity-scan", metavar="IMAGE",
                    help="check every block of IMAGE against its stored tree on the GPU (ROOT or --label follows)")
    ap.add_argument("--label", help="--verity-scan: N,OFF,sha256:ROOT in place of the three values")
    ap.add_argument("--data-blocks", type=int, help="--verity-verify / --verity-scan: 512-byte data blocks")
    ap.add_argument("--hash-offset", type=int,
                    help="--verity-verify / --verity-scan: where the tree starts in IMAGE")
    ap.add_argument("--diff", action="store_true", help="compare the chunk sets of two files")
    ap.add_argument("--tree", action="store_true", help="the inode tree instead of the chunk set")
    args = ap.parse_args(argv)
    if args.check:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: before the library)
        except ImportError:
            pass
        try:
            rep = check(args.check, args.dict, args.chunk_size, args.digester, retire=args.retire,
                        save_dict=args.save_dict, distill=args.distill, merge_blob_ids=args.merge_blob_ids)
        except (NgpuError, ValueError, OSError) as e:
            print(f"check: {e}", file=sys.stderr)
            return 2
        json.dump(rep, sys.stdout, indent=1)
        print()
        return 1 if rep["bad"] else 0
    if args.save_dict:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: before the library)
        except ImportError:
            pass
        try:
            rep = save_dict(args.save_dict, args.dict, args.chunk_size, args.digester, retire=args.retire,
                            distill=args.distill, merge_blob_ids=args.merge_blob_ids)
        except (NgpuError, ValueError, OSError) as e:
            print(f"save-dict: {e}", file=sys.stderr)
            return 2
        json.dump(rep, sys.stdout, indent=1)
        print()
        return 0
    if args.verity_scan:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: before the library)
        except ImportError:
            pass
        from ._lib import parse_verity_label
        some = args.data_blocks is not None or args.hash_offset is not None or bool(args.files)
        three = args.data_blocks is not None and args.hash_offset is not None and len(args.files) == 1
        if (args.label is not None) == some or (some and not three):
            ap.error("--verity-scan takes --data-blocks N --hash-offset OFF ROOT, or --label LABEL")
        try:
            v = parse_verity_label(args.label) if args.label is not None else \
                {"data_blocks": args.data_blocks, "hash_offset": args.hash_offset, "root": args.files[0]}
            rep = verity_scan(args.verity_scan, v["data_blocks"], v["hash_offset"], v["root"])
        except (NgpuError, ValueError, OSError) as e:
            print(f"verity: {e}", file=sys.stderr)
            return 2
        json.dump(rep, sys.stdout, indent=1)
        print()
        return 1 if rep["bad"] else 0
    if args.verity or args.verity_verify:
        try:
            import torch  # noqa: F401  (one HIP runtime per process: before the library)
        except ImportError:
            pass
        from ._lib import verity_options_line
        try:
            if args.verity:
                print(verity_options_line(verity(args.verity, args.append)))
                return 0
            if args.data_blocks is None or args.hash_offset is None or len(args.files) != 1:
                ap.error("--verity-verify takes --data-blocks N --hash-offset OFF ROOT")
            found = verity_verify(args.verity_verify, args.data_blocks, args.hash_offset, args.files[0])
        except (NgpuError, ValueError, OSError) as e:
            print(f"verity: {e}", file=sys.stderr)
            return 2
        for line in found:
            print(line)
        if not found:
            print(f"verity ok: {args.data_blocks} data blocks, root {args.files[0].lower()}")
        return 1 if found else 0
    if not args.files:
        ap.error("no file given")
    if args.tree:
        dumps = [tree(open(f, "rb").read()) for f in args.files]
    else:
        dumps = [canonical(load_bootstrap(open(f, "rb").read())) for f in args.files]
    if args.diff:
        if len(dumps) != 2:
            ap.error("--diff takes two files")
        d = tree_diff(*dumps) if args.tree else diff(*dumps)
        for sign, k in d:
            print(sign, *(k if isinstance(k, tuple) else (k,)))
        return 1 if d else 0
    for dmp in dumps:
        json.dump(dmp, sys.stdout, indent=1)
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
