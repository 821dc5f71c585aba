"""nydus_gpu — MI355X chunk digest + dedup engine for the nydus conversion path.

Python view of libnydusgpu.so (C ABI in include/nydus_gpu.h).  The engine
replaces the digest/dedup stage that pkg/converter hands to
`nydus-image create` (pkg/converter/tool/builder.go:148-178).
"""
from ._lib import (CHECK_BAD_DTYPE, CHECK_REASONS, CHUNK_DTYPE, COMPRESSORS, DEFAULT_DICT, DICT, DICT_PLACE_DTYPE, DICT_SAVE_NO_BLOB_TABLE, DICT_DISTILL_KEEP_BLOBS, DICT_DISTILL_MERGE_BLOB_IDS, NgpuDictDistillInfo, DIGESTED, DIGESTERS,  # noqa: F401
                   ECANCELED, EDEVICE, EFORMAT, EINVAL, EIO, ENODEV, EUNSUPP, UNHASHED,
                   ENOTFOUND, EXPORTS, FLAG_GRID_STAGES, FLAG_NO_BATCH, HIT_DTYPE, FdWriter, INTRA, KIND_NAMES, LAYER_STATS_DTYPE, MISS, NEW,
                   RESULT_DTYPE, TOC_ENTRY_DTYPE, ChunkDict, Engine, Node, NODE_DICT_PARTITION,
                   NODE_DICT_REPLICATE, NODE_EXCHANGE_COPY, NODE_EXCHANGE_ROUTED, NODE_STEP_RCCL, NgpuError, blob_write, chunk_table, dict_save_layout,
                   lib, merge, rafs_dump, verity_label, verity_layout, verity_options_line, parse_verity_label, VERITY_BAD_DTYPE, VERITY_REASONS, ref_chunk_read, route_digests, route_hits, tar_chunks, unpack,
                   unpack_entry)

__all__ = ["Engine", "Node", "NODE_DICT_PARTITION", "NODE_DICT_REPLICATE", "NODE_EXCHANGE_COPY", "NODE_EXCHANGE_ROUTED", "NODE_STEP_RCCL",
           "route_digests", "route_hits", "ref_chunk_read", "ChunkDict", "DEFAULT_DICT", "NgpuError", "tar_chunks", "chunk_table", "lib", "CHUNK_DTYPE",
           "RESULT_DTYPE", "DICT_PLACE_DTYPE", "DICT_SAVE_NO_BLOB_TABLE", "DICT_DISTILL_KEEP_BLOBS", "DICT_DISTILL_MERGE_BLOB_IDS", "NgpuDictDistillInfo", "dict_save_layout", "HIT_DTYPE", "MISS", "NEW", "INTRA", "DICT", "DIGESTED", "UNHASHED", "KIND_NAMES", "DIGESTERS", "EXPORTS",
           "COMPRESSORS", "TOC_ENTRY_DTYPE", "FdWriter", "blob_write", "unpack_entry", "unpack", "merge", "rafs_dump",
           "CHECK_BAD_DTYPE", "CHECK_REASONS", "verity_label", "verity_layout", "verity_options_line", "parse_verity_label", "VERITY_BAD_DTYPE", "VERITY_REASONS", "FLAG_GRID_STAGES", "FLAG_NO_BATCH", "EINVAL", "EFORMAT", "ENODEV", "EUNSUPP", "ENOTFOUND", "ECANCELED", "EDEVICE", "EIO"]
