"""kmerhash_amd: MI355X (gfx950) open-addressing k-mer hash tables behind the ParBLiSS/kmerhash table API.

The product is libkmerhash_amd.so (hand-written HIP, C-ABI in include/kmerhash_amd.h); this package is
the thin host-side mirror of the reference's interface for Python callers plus workload generators.
"""
from .table import (hashmap_robinhood_doubling, hashmap_linearprobe_doubling, hash_batch, HASHES,  # noqa: F401
                    KhError, KhLogicError, KhRetry)
from .wide import hashmap_robinhood_doubling_wide, hashmap_robinhood_doubling_wide_stream, hash_batch_wide, kmers128_from_sequence, kmers128_from_fastq  # noqa: F401
from .index import KmerPositionIndex, WideKmerPositionIndex  # noqa: F401
from .kmers import minimizers_from_sequence, minimizers_from_fastq  # noqa: F401
from .kmers import syncmers_from_sequence, syncmers_from_fastq, is_syncmer  # noqa: F401
from .kmers import stamp_strand, unstamp, anchors_from_csr, chain_anchors, chain_edits, chain_cigars, cigar_string, chain_ends, read_cigar, extended_intervals  # noqa: F401
from .kmers import select_chains, select_table, ChainSelect  # noqa: F401
from .kmers import chain_records, cigar_text, write_paf, paf_lines, ChainRecords, Mapping  # noqa: F401
from .kmers import group_anchors, AnchorGroups  # noqa: F401
from .kmers import pair_chains, pair_mapping, PairSelect  # noqa: F401
from .kmers import rescue_mates, rescue_requests, MateRescue, RESCUE_NONE, RESCUE_OVER  # noqa: F401
from .targets import Targets, TARGET_NONE  # noqa: F401
from .sam import record_diffs, oriented_rows, sam_header, sam_lines, write_sam, write_sam_pairs, write_sam_rescued, RecordDiffs  # noqa: F401
from .sam import names_csr, sam_line_columns, sam_lines_text, sam_text, write_sam_bytes, SamText, LineColumns  # noqa: F401
from .fastq import fastq_records, pack_rows, read_fastq, FastqRecords, Reads  # noqa: F401
from .wide import syncmers128_from_sequence, syncmers128_from_fastq, is_syncmer128  # noqa: F401
from .dist_index import ShardedKmerPositionIndex, IndexGpuBackend, WideIndexGpuBackend  # noqa: F401
from . import workloads  # noqa: F401

__all__ = ["hashmap_robinhood_doubling", "hashmap_linearprobe_doubling", "hash_batch", "HASHES", "KhError",
           "KhLogicError", "KhRetry", "workloads", "hashmap_robinhood_doubling_wide", "hashmap_robinhood_doubling_wide_stream", "hash_batch_wide", "kmers128_from_sequence",
           "kmers128_from_fastq", "KmerPositionIndex", "WideKmerPositionIndex", "minimizers_from_sequence", "minimizers_from_fastq",
           "ShardedKmerPositionIndex", "IndexGpuBackend", "WideIndexGpuBackend", "syncmers_from_sequence", "syncmers_from_fastq", "is_syncmer",
           "syncmers128_from_sequence", "syncmers128_from_fastq", "is_syncmer128", "stamp_strand", "unstamp", "anchors_from_csr", "chain_anchors",
           "chain_edits", "chain_cigars", "cigar_string", "chain_ends", "read_cigar", "extended_intervals",
           "select_chains", "select_table", "ChainSelect",
           "chain_records", "cigar_text", "write_paf", "paf_lines", "ChainRecords", "Mapping",
           "group_anchors", "AnchorGroups", "Targets", "TARGET_NONE",
           "record_diffs", "oriented_rows", "sam_header", "sam_lines", "write_sam", "RecordDiffs",
           "pair_chains", "pair_mapping", "PairSelect", "write_sam_pairs",
           "rescue_mates", "rescue_requests", "MateRescue", "RESCUE_NONE", "RESCUE_OVER", "write_sam_rescued",
           "names_csr", "sam_line_columns", "sam_lines_text", "sam_text", "write_sam_bytes", "SamText", "LineColumns",
           "fastq_records", "pack_rows", "read_fastq", "FastqRecords", "Reads"]
