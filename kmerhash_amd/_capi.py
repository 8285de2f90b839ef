"""ctypes binding of include/kmerhash_amd.h (libkmerhash_amd.so).  No fallback: if the HIP library is
missing or no GPU is usable, importing works but every table constructor raises."""
import ctypes as C
import os

from .build import LIB

KH_OK, KH_ERR_INVALID, KH_ERR_NOMEM, KH_ERR_FULL, KH_ERR_PROBE_OVERFLOW, KH_ERR_HIP, KH_ERR_UNSUPPORTED, KH_ERR_RETRY = range(8)
KH_INS_REDUCE_PLUS, KH_INS_REPEATABLE = 1, 2
KH_REDUCE_PLUS, KH_REDUCE_MIN, KH_REDUCE_MAX, KH_REDUCE_OR = range(4)
KH_INS_REDUCE_OP_SHIFT = 2
REDUCE_OPS = {"plus": KH_REDUCE_PLUS, "min": KH_REDUCE_MIN, "max": KH_REDUCE_MAX, "or": KH_REDUCE_OR}


def reduce_op(op):
    """name of a Reducer -> kh_reduce_op; anything else is refused here, before any call into the library"""
    if not isinstance(op, str) or op not in REDUCE_OPS:
        raise ValueError("reduce operation must be one of 'plus', 'min', 'max', 'or', got %r" % (op,))
    return REDUCE_OPS[op]


def ins_flags(reduce_plus=False, repeatable=False, reduce=None):
    """flags of kh_insert_begin_ex / kh_wide_insert_begin_ex: KH_INS_REDUCE(op) | KH_INS_REPEATABLE"""
    flags = KH_INS_REPEATABLE if repeatable else 0
    if reduce is not None:
        op = reduce_op(reduce)
        if reduce_plus and op != KH_REDUCE_PLUS:
            raise ValueError("reduce_plus=True contradicts reduce=%r" % (reduce,))
        return flags | KH_INS_REDUCE_PLUS | (op << KH_INS_REDUCE_OP_SHIFT)
    return flags | (KH_INS_REDUCE_PLUS if reduce_plus else 0)

KH_KIND_ROBINHOOD, KH_KIND_LINEARPROBE = 0, 1
KH_HASH_IDENTITY, KH_HASH_MURMUR3_X86_128_LO64, KH_HASH_MURMUR3_X64_128_H0, KH_HASH_FARM64 = 0, 1, 2, 3
KH_MEM_HOST, KH_MEM_DEVICE = 0, 1
KH_XF_IDENTITY, KH_XF_DNA_LEX_LESS = 0, 1

STATUS_NAMES = {0: "KH_OK", 1: "KH_ERR_INVALID", 2: "KH_ERR_NOMEM", 3: "KH_ERR_FULL", 4: "KH_ERR_PROBE_OVERFLOW",
                5: "KH_ERR_HIP", 6: "KH_ERR_UNSUPPORTED", 7: "KH_ERR_RETRY"}

# every symbol include/kmerhash_amd.h declares (tests check the library exports each one)
SYMBOLS = [
    "kh_create", "kh_destroy", "kh_set_stream", "kh_set_key_transform", "kh_get_key_transform", "kh_hash_batch_transformed", "kh_shard_permute_transformed", "kh_last_error", "kh_size", "kh_capacity", "kh_get_load_thresholds",
    "kh_set_min_load_factor", "kh_set_max_load_factor", "kh_get_load_factors", "kh_clear", "kh_reserve", "kh_rehash",
    "kh_insert", "kh_insert_pairs", "kh_insert_one", "kh_update", "kh_insert_reduce_plus", "kh_insert_begin", "kh_insert_begin_ex", "kh_insert_feed", "kh_insert_end", "kh_insert_abort", "kh_count", "kh_find", "kh_find_compact", "kh_find_compact_pairs",
    "kh_erase", "kh_erase_one", "kh_to_vector", "kh_export_info", "kh_export_slots", "kh_export_raw_slots", "kh_displacement_histogram",
    "kh_hash_batch", "kh_shard_permute", "kh_shard_plan_create", "kh_shard_plan_permute", "kh_shard_plan_permute_global", "kh_shard_plan_offsets", "kh_shard_plan_destroy", "kh_profile_enable", "kh_profile_reset", "kh_profile_query", "kh_profile_dump",
    "kh_kmers_from_sequence", "kh_kmers_from_fastq", "kh_hll_create", "kh_hll_destroy", "kh_hll_set_stream", "kh_hll_update", "kh_hll_update_via_hashval",
    "kh_hll_merge", "kh_hll_clear", "kh_hll_registers", "kh_hll_estimate", "kh_hll_estimate_registers", "kh_release_cached_memory", "kh_version",
    # wide keys (16-byte keys, k <= 64)
    "kh_wide_create", "kh_wide_destroy", "kh_wide_set_stream", "kh_wide_last_error", "kh_wide_size", "kh_wide_capacity", "kh_wide_get_load_factors",
    "kh_wide_set_min_load_factor", "kh_wide_set_max_load_factor", "kh_wide_clear", "kh_wide_reserve", "kh_wide_rehash", "kh_wide_insert",
    "kh_wide_insert_reduce_plus", "kh_wide_count", "kh_wide_find", "kh_wide_find_compact", "kh_wide_erase", "kh_wide_to_vector",
    "kh_wide_export_info", "kh_wide_displacement_histogram", "kh_wide_hash_batch", "kh_kmers128_from_sequence", "kh_kmers128_from_fastq",
    # wide keys across GPUs: the streamed insert and the stable partition by destination rank
    "kh_wide_insert_begin_ex", "kh_wide_insert_feed", "kh_wide_insert_end", "kh_wide_insert_abort", "kh_wide_shard_permute",
    # value-range operations (spectrum, select and erase by value), both key widths
    "kh_value_histogram", "kh_select_values", "kh_erase_values", "kh_wide_value_histogram", "kh_wide_select_values", "kh_wide_erase_values",
    # HyperLogLog over 16-byte keys and straight from text (k = 1..64)
    "kh_hll_update_wide", "kh_hll_update_from_sequence", "kh_hll_update_from_fastq",
    # reducer inserts beyond std::plus (min, max, bit-or), both key widths
    "kh_insert_reduce", "kh_wide_insert_reduce",
    # k-mer position index (all occurrences per k-mer) and the front end that keeps window offsets
    "kh_kmers_from_sequence_pos", "kh_kmers_from_fastq_pos",
    "kh_index_create", "kh_index_destroy", "kh_index_set_stream", "kh_index_last_error", "kh_index_clear", "kh_index_build",
    "kh_index_build_from_sequence", "kh_index_build_from_fastq", "kh_index_size", "kh_index_total", "kh_index_capacity", "kh_index_export",
    "kh_index_count", "kh_index_find", "kh_index_profile_enable", "kh_index_profile_dump",
    # position index over 16-byte k-mers (k <= 64) and its front end
    "kh_kmers128_from_sequence_pos", "kh_kmers128_from_fastq_pos",
    "kh_wide_index_create", "kh_wide_index_destroy", "kh_wide_index_set_stream", "kh_wide_index_last_error", "kh_wide_index_clear", "kh_wide_index_build",
    "kh_wide_index_build_from_sequence", "kh_wide_index_build_from_fastq", "kh_wide_index_size", "kh_wide_index_total", "kh_wide_index_capacity",
    "kh_wide_index_export", "kh_wide_index_export_info", "kh_wide_index_count", "kh_wide_index_find", "kh_wide_index_profile_enable", "kh_wide_index_profile_dump",
    # changing a built index: append batches, erase keys, erase by occurrence count (both key widths)
    "kh_index_append", "kh_index_append_from_sequence", "kh_index_append_from_fastq", "kh_index_erase", "kh_index_erase_counts",
    "kh_wide_index_append", "kh_wide_index_append_from_sequence", "kh_wide_index_append_from_fastq", "kh_wide_index_erase", "kh_wide_index_erase_counts",
    # (w,k)-minimizer sampling and the position index over the sampled k-mers
    "kh_minimizers_from_sequence", "kh_minimizers_from_fastq", "kh_index_build_from_minimizers", "kh_index_append_from_minimizers",
    # a permuted CSR back into query order (the last step of a sharded index find)
    "kh_csr_unpermute",
    # closed-syncmer sampling (both key widths), the context-free keep test and the position index over the kept k-mers
    "kh_syncmers_from_sequence", "kh_syncmers_from_fastq", "kh_syncmers128_from_sequence", "kh_syncmers128_from_fastq",
    "kh_syncmer_mask", "kh_wide_syncmer_mask", "kh_index_build_from_syncmers", "kh_index_append_from_syncmers",
    "kh_wide_index_build_from_syncmers", "kh_wide_index_append_from_syncmers",
    # strand of a window position, stranded indexes (a strand bit per occurrence), a CSR of hits into flat anchors
    "kh_stamp_strand", "kh_index_set_stranded", "kh_wide_index_set_stranded", "kh_anchors_from_csr",
    # collinear chains per segment (read) from flat anchors
    "kh_chain_anchors",
    # edit distance of every chain link against the two texts
    "kh_chain_edits",
    # alignment operations (run-length CIGAR rows) of every chain link, by traceback
    "kh_chain_cigars",
    # both ends of every chain extended to the ends of its read or to a soft clip
    "kh_chain_ends",
    # primary / secondary chains per read and a mapping quality per primary
    "kh_chain_select",
    # one alignment record per chain from the link rows, end rows and clips; a run CSR as CIGAR text
    "kh_chain_records",
    "kh_cigar_text",
    # the anchors of every read regrouped by the target (contig) they fall in
    "kh_anchor_targets",
    # SAM output: the cs / MD string of every record row, byte ranges in reference orientation (SEQ, QUAL)
    "kh_record_diffs",
    "kh_oriented_rows",
    # paired reads: the concordant chain pair of two mates, proper flag, pair quality, template length
    "kh_pair_chains",
    # mate rescue: a mate without a row aligned end to end inside the window its partner allows
    "kh_mate_rescue",
    # SAM lines on the device: the text of the alignment lines from line columns and byte CSRs
    "kh_sam_lines",
    # FASTQ in: the record structure of a FASTQ text, and byte rows gathered to given places
    "kh_fastq_records", "kh_pack_rows",
]

_lib = None
vp, u64, u32, i32, f32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_float
pu64 = C.POINTER(C.c_uint64)


class KhError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), msg))
        self.status = status


class KhRetry(KhError):
    """kh_insert_end of a repeatable streamed insert: the speculative partition did not hold; feed the same pieces again"""


class KhLogicError(KhError):
    """mirrors std::logic_error thrown by the reference LP table (hashmap_linearprobe.hpp:408,503)"""


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RuntimeError("libkmerhash_amd.so is not built (run `python -m kmerhash_amd.build` / __graft_entry__.build()); "
                           "there is no CPU fallback")
    L = C.CDLL(LIB)
    L.kh_version.restype = C.c_char_p
    L.kh_last_error.restype = C.c_char_p
    L.kh_last_error.argtypes = [vp]
    L.kh_create.argtypes = [C.POINTER(vp), i32, u32, u32, i32, u64, u64, f32, f32, i32]
    L.kh_destroy.argtypes = [vp]
    L.kh_set_stream.argtypes = [vp, vp]
    L.kh_set_key_transform.argtypes = [vp, i32, u32]
    L.kh_get_key_transform.argtypes = [vp, C.POINTER(i32), C.POINTER(u32)]
    L.kh_hash_batch_transformed.argtypes = [i32, u64, i32, u32, vp, u64, i32, vp, i32, vp]
    L.kh_shard_permute_transformed.argtypes = [i32, u64, i32, u32, u32, vp, vp, u64, vp, vp, vp, i32, vp]
    L.kh_size.argtypes = [vp, pu64]
    L.kh_capacity.argtypes = [vp, pu64]
    L.kh_get_load_thresholds.argtypes = [vp, pu64, pu64]
    L.kh_set_min_load_factor.argtypes = [vp, f32]
    L.kh_set_max_load_factor.argtypes = [vp, f32]
    L.kh_get_load_factors.argtypes = [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]
    L.kh_clear.argtypes = [vp]
    L.kh_reserve.argtypes = [vp, u64]
    L.kh_rehash.argtypes = [vp, u64]
    L.kh_insert.argtypes = [vp, vp, vp, u64, i32, pu64]
    L.kh_insert_pairs.argtypes = [vp, vp, u64, i32, pu64]
    L.kh_insert_one.argtypes = [vp, u64, u32, pu64]
    L.kh_update.argtypes = [vp, vp, vp, u64, i32, pu64]
    L.kh_insert_reduce_plus.argtypes = [vp, vp, vp, u64, i32, pu64]
    L.kh_insert_reduce.argtypes = [vp, vp, vp, u64, i32, i32, pu64]
    L.kh_wide_insert_reduce.argtypes = [vp, vp, vp, u64, i32, i32, pu64]
    L.kh_insert_begin.argtypes = [vp, u64, i32]
    L.kh_insert_begin_ex.argtypes = [vp, u64, u32]
    L.kh_shard_plan_create.argtypes = [C.POINTER(vp), i32, u64, i32, u32, u32, vp, u64, u32, pu64, pu64, i32, vp]
    L.kh_shard_plan_permute.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.kh_shard_plan_permute_global.argtypes = [vp, u32, vp, vp, vp, vp, vp]
    L.kh_shard_plan_offsets.argtypes = [vp, pu64]
    L.kh_shard_plan_destroy.argtypes = [vp]
    L.kh_shard_plan_destroy.restype = None
    L.kh_insert_feed.argtypes = [vp, vp, vp, u64, i32]
    L.kh_insert_end.argtypes = [vp, pu64]
    L.kh_insert_abort.argtypes = [vp]
    L.kh_count.argtypes = [vp, vp, u64, i32, vp]
    L.kh_find.argtypes = [vp, vp, u64, i32, vp, vp, pu64]
    L.kh_find_compact.argtypes = [vp, vp, u64, i32, vp, vp, pu64]
    L.kh_find_compact_pairs.argtypes = [vp, vp, u64, i32, vp, pu64]
    L.kh_erase.argtypes = [vp, vp, u64, i32, pu64]
    L.kh_erase_one.argtypes = [vp, u64, pu64]
    L.kh_to_vector.argtypes = [vp, vp, vp, pu64]
    L.kh_export_info.argtypes = [vp, vp]
    L.kh_export_slots.argtypes = [vp, vp, vp]
    L.kh_export_raw_slots.argtypes = [vp, vp]
    L.kh_displacement_histogram.argtypes = [vp, vp]
    L.kh_hash_batch.argtypes = [i32, u64, vp, u64, i32, vp, i32, vp]
    L.kh_shard_permute.argtypes = [i32, u64, u32, vp, vp, u64, vp, vp, vp, i32, vp]
    L.kh_release_cached_memory.argtypes = [i32]
    L.kh_kmers_from_sequence.argtypes = [vp, u64, u32, i32, i32, vp, pu64, i32, vp]
    L.kh_kmers_from_fastq.argtypes = [vp, u64, u32, i32, i32, vp, pu64, i32, vp]
    L.kh_hll_create.argtypes = [C.POINTER(vp), u32, u32, i32, u64, i32]
    L.kh_hll_destroy.argtypes = [vp]
    L.kh_hll_set_stream.argtypes = [vp, vp]
    L.kh_hll_update.argtypes = [vp, vp, u64, i32]
    L.kh_hll_update_via_hashval.argtypes = [vp, vp, u64, i32]
    L.kh_hll_update_wide.argtypes = [vp, vp, u64, i32]
    L.kh_hll_update_from_sequence.argtypes = [vp, vp, u64, u32, i32, i32, pu64]
    L.kh_hll_update_from_fastq.argtypes = [vp, vp, u64, u32, i32, i32, pu64]
    L.kh_hll_merge.argtypes = [vp, vp]
    L.kh_hll_clear.argtypes = [vp]
    L.kh_hll_registers.argtypes = [vp, vp]
    L.kh_hll_estimate.argtypes = [vp, C.POINTER(C.c_double)]
    L.kh_hll_estimate_registers.argtypes = [vp, u32, C.POINTER(C.c_double)]
    L.kh_profile_enable.argtypes = [vp, i32]
    L.kh_profile_reset.argtypes = [vp]
    L.kh_profile_query.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), pu64]
    L.kh_profile_dump.argtypes = [vp, C.c_char_p, u64]
    L.kh_wide_last_error.restype = C.c_char_p
    L.kh_wide_last_error.argtypes = [vp]
    L.kh_wide_create.argtypes = [C.POINTER(vp), i32, i32, u64, u64, f32, f32, i32]
    L.kh_wide_destroy.argtypes = [vp]
    L.kh_wide_set_stream.argtypes = [vp, vp]
    L.kh_wide_size.argtypes = [vp, pu64]
    L.kh_wide_capacity.argtypes = [vp, pu64]
    L.kh_wide_get_load_factors.argtypes = [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)]
    L.kh_wide_set_min_load_factor.argtypes = [vp, f32]
    L.kh_wide_set_max_load_factor.argtypes = [vp, f32]
    L.kh_wide_clear.argtypes = [vp]
    L.kh_wide_reserve.argtypes = [vp, u64]
    L.kh_wide_rehash.argtypes = [vp, u64]
    L.kh_wide_insert.argtypes = [vp, vp, vp, u64, i32, pu64]
    L.kh_wide_insert_reduce_plus.argtypes = [vp, vp, vp, u64, i32, pu64]
    L.kh_wide_count.argtypes = [vp, vp, u64, i32, vp]
    L.kh_wide_find.argtypes = [vp, vp, u64, i32, vp, vp, pu64]
    L.kh_wide_find_compact.argtypes = [vp, vp, u64, i32, vp, vp, pu64]
    L.kh_wide_erase.argtypes = [vp, vp, u64, i32, pu64]
    L.kh_wide_to_vector.argtypes = [vp, vp, vp, pu64]
    L.kh_wide_export_info.argtypes = [vp, vp]
    L.kh_wide_displacement_histogram.argtypes = [vp, vp]
    L.kh_wide_hash_batch.argtypes = [i32, u64, vp, u64, i32, vp, i32, vp]
    L.kh_wide_insert_begin_ex.argtypes = [vp, u64, u32]
    L.kh_wide_insert_feed.argtypes = [vp, vp, vp, u64, i32]
    L.kh_wide_insert_end.argtypes = [vp, pu64]
    L.kh_wide_insert_abort.argtypes = [vp]
    L.kh_wide_shard_permute.argtypes = [i32, u64, u32, vp, vp, u64, vp, vp, vp, i32, vp]
    L.kh_kmers128_from_sequence.argtypes = [vp, u64, u32, i32, i32, vp, pu64, i32, vp]
    L.kh_kmers128_from_fastq.argtypes = [vp, u64, u32, i32, i32, vp, pu64, i32, vp]
    for pre in ("kh_", "kh_wide_"):
        getattr(L, pre + "value_histogram").argtypes = [vp, u32, vp]
        getattr(L, pre + "select_values").argtypes = [vp, u32, u32, i32, vp, vp, u64, pu64]
        getattr(L, pre + "erase_values").argtypes = [vp, u32, u32, pu64]
    L.kh_kmers_from_sequence_pos.argtypes = [vp, u64, u32, i32, i32, vp, vp, pu64, i32, vp]
    L.kh_kmers_from_fastq_pos.argtypes = [vp, u64, u32, i32, i32, vp, vp, pu64, i32, vp]
    L.kh_kmers128_from_sequence_pos.argtypes = [vp, u64, u32, i32, i32, vp, vp, pu64, i32, vp]
    L.kh_kmers128_from_fastq_pos.argtypes = [vp, u64, u32, i32, i32, vp, vp, pu64, i32, vp]
    for pre in ("kh_index_", "kh_wide_index_"):      # one contract, two key widths
        getattr(L, pre + "last_error").restype = C.c_char_p
        getattr(L, pre + "last_error").argtypes = [vp]
        getattr(L, pre + "create").argtypes = [C.POINTER(vp), i32, u64, f32, f32, i32]
        getattr(L, pre + "destroy").argtypes = [vp]
        getattr(L, pre + "set_stream").argtypes = [vp, vp]
        getattr(L, pre + "clear").argtypes = [vp]
        getattr(L, pre + "build").argtypes = [vp, vp, vp, u64, i32]
        getattr(L, pre + "build_from_sequence").argtypes = [vp, vp, u64, u32, i32, i32]
        getattr(L, pre + "build_from_fastq").argtypes = [vp, vp, u64, u32, i32, i32]
        getattr(L, pre + "size").argtypes = [vp, pu64]
        getattr(L, pre + "total").argtypes = [vp, pu64]
        getattr(L, pre + "capacity").argtypes = [vp, pu64]
        getattr(L, pre + "export").argtypes = [vp, vp, vp, vp]
        getattr(L, pre + "count").argtypes = [vp, vp, u64, i32, vp]
        getattr(L, pre + "find").argtypes = [vp, vp, u64, i32, vp, vp, u64, pu64]
        getattr(L, pre + "profile_enable").argtypes = [vp, i32]
        getattr(L, pre + "profile_dump").argtypes = [vp, C.c_char_p, u64]
        getattr(L, pre + "append").argtypes = [vp, vp, vp, u64, i32]
        getattr(L, pre + "append_from_sequence").argtypes = [vp, vp, u64, u32, i32, i32, u32]
        getattr(L, pre + "append_from_fastq").argtypes = [vp, vp, u64, u32, i32, i32, u32]
        getattr(L, pre + "erase").argtypes = [vp, vp, u64, i32, pu64, pu64]
        getattr(L, pre + "erase_counts").argtypes = [vp, u32, u32, pu64, pu64]
    L.kh_wide_index_export_info.argtypes = [vp, vp]
    L.kh_minimizers_from_sequence.argtypes = [vp, u64, u32, u32, i32, i32, u64, i32, vp, vp, u64, pu64, i32, vp]
    L.kh_minimizers_from_fastq.argtypes = [vp, u64, u32, u32, i32, i32, u64, i32, vp, vp, u64, pu64, i32, vp]
    L.kh_index_build_from_minimizers.argtypes = [vp, vp, u64, u32, u32, i32, i32, u64, i32, i32]
    L.kh_index_append_from_minimizers.argtypes = [vp, vp, u64, u32, u32, i32, i32, u64, i32, i32, u32]
    L.kh_csr_unpermute.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, pu64, i32, vp]
    for s in ("kh_syncmers_from_sequence", "kh_syncmers_from_fastq", "kh_syncmers128_from_sequence", "kh_syncmers128_from_fastq"):
        getattr(L, s).argtypes = [vp, u64, u32, u32, i32, i32, u64, i32, vp, vp, u64, pu64, i32, vp]
    L.kh_syncmer_mask.argtypes = [vp, u64, u32, u32, i32, i32, u64, i32, vp, i32, vp]
    L.kh_wide_syncmer_mask.argtypes = [vp, u64, u32, u32, i32, i32, u64, i32, vp, i32, vp]
    for pre in ("kh_index_", "kh_wide_index_"):
        getattr(L, pre + "build_from_syncmers").argtypes = [vp, vp, u64, u32, u32, i32, i32, u64, i32, i32]
        getattr(L, pre + "append_from_syncmers").argtypes = [vp, vp, u64, u32, u32, i32, i32, u64, i32, i32, u32]
    L.kh_stamp_strand.argtypes = [vp, u64, u32, vp, u64, u32, i32, vp, pu64, i32, vp]
    L.kh_index_set_stranded.argtypes = [vp, i32]
    L.kh_wide_index_set_stranded.argtypes = [vp, i32]
    L.kh_anchors_from_csr.argtypes = [vp, vp, u64, vp, u64, i32, vp, vp, vp, i32, vp]
    L.kh_chain_anchors.argtypes = [vp, vp, vp, u64, vp, u64, u32, u32, u32, u32, i32, u32, i32, vp, vp, vp, vp, vp, vp, vp, u64, pu64, i32, vp]
    L.kh_chain_edits.argtypes = [vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, u64, u64, u32, u32, i32, vp, vp, vp, i32, vp]
    L.kh_chain_cigars.argtypes = [vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, u64, u64, u32, vp, i32, vp, vp, u64, pu64, vp, vp, i32, vp]
    L.kh_chain_ends.argtypes = [vp, u64, vp, u64, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp, u64, pu64, i32, vp]
    L.kh_chain_select.argtypes = [vp, vp, vp, vp, u64, vp, u64, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.kh_chain_records.argtypes = [vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, u32, u32, i32] + [vp] * 11 + [u64, pu64, i32, vp]
    L.kh_cigar_text.argtypes = [vp, u64, vp, u64, i32, vp, vp, u64, pu64, i32, vp]
    L.kh_record_diffs.argtypes = [vp, u64, vp, u64, u32, vp, vp, u64, vp, vp, vp, vp, vp, u64, u32, i32, vp, vp, vp, u64, pu64, i32, vp]
    L.kh_oriented_rows.argtypes = [vp, u64, vp, vp, vp, u64, u32, i32, vp, vp, u64, pu64, i32, vp]
    L.kh_pair_chains.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, vp, u64, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    L.kh_mate_rescue.argtypes = [vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, u64, u32, i32, vp, vp, vp, vp, vp, vp, u64, pu64, i32, vp]
    L.kh_sam_lines.argtypes = [vp, vp, u64, u64] * 7 + [vp] * 19 + [u64, i32, vp, vp, u64, pu64, i32, vp]
    L.kh_fastq_records.argtypes = [vp, u64, u32, i32, vp, vp, vp, vp, vp, vp, u64, pu64, pu64, C.POINTER(C.c_uint32), i32, vp]
    L.kh_pack_rows.argtypes = [vp, u64, vp, vp, vp, u64, i32, i32, vp, u64, i32, vp]
    L.kh_anchor_targets.argtypes =[vp, vp, vp, u64, vp, u64, vp, vp, u64, u32, i32] + [vp] * 8 + [pu64, i32, vp]
    for s in SYMBOLS:
        if s not in ("kh_version", "kh_last_error", "kh_wide_last_error", "kh_index_last_error", "kh_wide_index_last_error"):
            getattr(L, s).restype = i32
    _lib = L
    return L
