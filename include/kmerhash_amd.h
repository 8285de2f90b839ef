/* kmerhash_amd.h -- C-ABI of libkmerhash_amd.so: MI355X (gfx950) open-addressing k-mer hash tables.
 *
 * This is the drop-in boundary for ONE hot path of ParBLiSS/kmerhash: the batched
 * insert / find / count / erase of
 *     fsc::hashmap_robinhood_doubling   (reference include/kmerhash/hashmap_robinhood.hpp:124-126)
 *     fsc::hashmap_linearprobe_doubling (reference include/kmerhash/hashmap_linearprobe.hpp:96-98)
 * for 64-bit keys (2-bit packed k-mers, k <= 32) with 32-bit mapped values, and of the 64-bit hash
 * functors they are instantiated with.  Plain pointers and sizes only; no C++/torch types cross it.
 * The C++ template shim (include/kmerhash_amd/hashmap.hpp) and the Python host layer (kmerhash_amd/) are
 * thin callers of exactly these entry points; INTEGRATION.md shows the reference-side binding.
 *
 * Every function returns a kh_status; kh_last_error() gives the text of the last failure on a table.
 * A table is single-writer (like the reference: not thread safe); read-only batches may not overlap
 * a mutating batch.  All device work of a table is issued on its stream (kh_set_stream) and the
 * functions that return scalar results (n_inserted, n_found, ...) synchronise that stream.
 *
 * Pointer arguments marked [h|d] live in host or device memory as told by the kh_mem argument;
 * outputs live in the same space as the inputs of that call.  Device pointers must be valid on the
 * table's device.
 */
#ifndef KMERHASH_AMD_H_
#define KMERHASH_AMD_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kh_table kh_table;

typedef enum {
  KH_OK = 0,
  KH_ERR_INVALID = 1,        /* bad argument / unsupported key or value width */
  KH_ERR_NOMEM = 2,          /* device allocation failed */
  KH_ERR_FULL = 3,           /* LP: no slot left -- mirrors std::logic_error, hashmap_linearprobe.hpp:408,503 */
  KH_ERR_PROBE_OVERFLOW = 4, /* RH probe distance would reach 128: the reference asserts (hashmap_robinhood.hpp:556)
                                or silently corrupts under -DNDEBUG; we refuse.  A call that re-lays the table out leaves it
                                unchanged: size, capacity, info bytes, keys and values (reducer inserts are rolled back).
                                A batch applied IN PLACE is applied key by key and keeps what was applied; the table stays a
                                consistent Robin Hood table and *n_inserted counts the keys inserted.
                                - a mid-size batch into a large table: every key is inserted whole or left out, and one is left
                                  out only if its own insertion would push an element to distance 128; the rest of the batch IS
                                  applied (also the reductions and updates of keys the table held).
                                - <= 16 keys: applied in batch order up to the first key that does not fit.  The keys BEFORE it
                                  stay applied (inserts, reductions, updates); that key and every key after it are refused
                                  together and leave no trace, even those that would fit.
                                kh_erase_one: see there.  (tests/test_gpu_refusals.py) */
  KH_ERR_HIP = 5,            /* a HIP runtime call failed (no GPU, launch failure, ...) */
  KH_ERR_UNSUPPORTED = 6,
  KH_ERR_RETRY = 7           /* kh_insert_end of a KH_INS_REPEATABLE streamed insert: its speculative partition did not hold for this
                                batch; nothing was inserted; feed the same pieces again after kh_insert_begin without that flag */
} kh_status;

typedef enum {
  KH_KIND_ROBINHOOD = 0,     /* fsc::hashmap_robinhood_doubling  : info 0x00 empty, 0x80|dist occupied (:137-163) */
  KH_KIND_LINEARPROBE = 1    /* fsc::hashmap_linearprobe_doubling: info 0x40 empty, 0x80 deleted, 0x00 normal (:109-139) */
} kh_kind;

typedef enum {
  KH_HASH_IDENTITY = 0,             /* fsc::hash::identity<T>      hash_new.hpp:135-166 */
  KH_HASH_MURMUR3_X86_128_LO64 = 1, /* fsc::hash::murmur3avx64<T>  murmurhash3_64_avx.hpp:1553-1651 (== murmur_x86, hash_new.hpp:218) */
  KH_HASH_MURMUR3_X64_128_H0 = 2,   /* fsc::hash::murmur<T>        hash_new.hpp:206-235 */
  KH_HASH_FARM64 = 3                /* fsc::hash::farm<T>          hash_new.hpp:309-328 (parity unpinned) */
} kh_hash;

typedef enum { KH_MEM_HOST = 0, KH_MEM_DEVICE = 1 } kh_mem;

/* Key transform in front of the hash and inside key equality: fsc::TransformedHash<Key, Hash, PreTransform> together with
 * fsc::TransformedComparator<Key, std::equal_to, PreTransform> (hash_new.hpp:387-1134; used with
 * bliss::kmer::transform::lex_less for "bimolecule" tables in which a k-mer and its reverse complement are one key,
 * test/unit/test_hashmap_robinhood_doubling.cpp:560-626).  The table stores the key bits of the FIRST occurrence, as the
 * reference does; find / to_vector return the stored bits. */
typedef enum {
  KH_XF_IDENTITY = 0,      /* bliss::transform::identity */
  KH_XF_DNA_LEX_LESS = 1   /* bliss::kmer::transform::lex_less on a 2-bit packed DNA k-mer (first base most significant, A0 C1 G2 T3):
                              the key stands for min(key, reverse complement).  kmerind's own packing is not part of the reference
                              tree: PARITY UNPINNED for the bit layout */
} kh_key_transform;

/* ---- lifetime: ctor (capacity=128, min_lf, max_lf)  hashmap_robinhood.hpp:218-233 / hashmap_linearprobe.hpp:191-206
 *      key_bytes must be 8 (every batch argument of a kh_table is u64[n]); 16-byte keys live in the separate kh_wtable below. */
kh_status kh_create(kh_table** out, kh_kind kind, uint32_t key_bytes /*8*/, uint32_t val_bytes /*4*/,
                    kh_hash hash, uint64_t seed /*43*/, uint64_t capacity /*128*/,
                    float min_load_factor, float max_load_factor, int device);
kh_status kh_destroy(kh_table* t);
/* Streams (DESIGN.md "Streams"): all device work of a handle is issued on the handle's stream.  A change of stream keeps earlier work
 *      ordered before later work: kh_set_stream waits for the old stream before it switches (the same stream again: nothing happens), so
 *      calls on one handle take effect in call order whichever streams they were issued under.  A call that reads a second handle
 *      (kh_hll_merge) is ordered after that handle's pending work.  Most calls return a scalar and have synchronised the stream when
 *      they return.  The calls that only queue their work, when given device memory, are: kh_count, kh_wide_count, kh_find with
 *      n_found == NULL, kh_insert_feed / kh_wide_insert_feed, kh_hash_batch / kh_hash_batch_transformed / kh_wide_hash_batch,
 *      kh_shard_plan_permute / _permute_global, and kh_hll_update / _update_via_hashval / _update_wide, kh_hll_update_from_sequence /
 *      _from_fastq with n_kmers == NULL, kh_hll_merge and kh_hll_clear.  For these the caller's input buffers must stay valid and
 *      unchanged, and the outputs are complete, only in the order of that stream: until work queued behind the call on the same
 *      stream runs, or the stream (or a later synchronising call on the handle) has been waited for. */
kh_status kh_set_stream(kh_table* t, void* hip_stream /* hipStream_t; NULL = default stream */);
/* the PreTransform of the table's TransformedHash / TransformedComparator; k = k-mer length (1..32) for KH_XF_DNA_LEX_LESS.
 * Only on an empty table (the reference fixes it at compile time). */
kh_status kh_set_key_transform(kh_table* t, kh_key_transform xf, uint32_t k);
kh_status kh_get_key_transform(const kh_table* t, kh_key_transform* xf, uint32_t* k);
const char* kh_last_error(const kh_table* t);

/* ---- scalar state: size() :406 / capacity() :287 / load factors :261-285 / clear :413 / reserve :421 / rehash :432 */
kh_status kh_size(const kh_table* t, uint64_t* out);
kh_status kh_capacity(const kh_table* t, uint64_t* out);
kh_status kh_get_load_thresholds(const kh_table* t, uint64_t* min_load, uint64_t* max_load);
kh_status kh_set_min_load_factor(kh_table* t, float f);
kh_status kh_set_max_load_factor(kh_table* t, float f);
kh_status kh_get_load_factors(const kh_table* t, float* min_lf, float* max_lf, float* current);
kh_status kh_clear(kh_table* t);
kh_status kh_reserve(kh_table* t, uint64_t n);
kh_status kh_rehash(kh_table* t, uint64_t buckets);

/* ---- batch insert == insert(Iter,Iter) / insert(vector const&)  hashmap_robinhood.hpp:633-717,
 *      hashmap_linearprobe.hpp:521-573.  First value wins; capacity follows the reference's doubling
 *      rule exactly (one doubling per insert call made while size >= max_load, duplicates included). */
kh_status kh_insert(kh_table* t, const void* keys /*[h|d] u64[n]*/, const void* vals /*[h|d] u32[n]*/,
                    uint64_t n, kh_mem where, uint64_t* n_inserted);
/* same, input as the reference's std::pair<uint64_t,uint32_t> array (16 B: key @0, value @8) */
kh_status kh_insert_pairs(kh_table* t, const void* pairs16 /*[h|d]*/, uint64_t n, kh_mem where, uint64_t* n_inserted);
/* insert(value_type const&) / insert(key, val): the single-key form (hashmap_robinhood.hpp:522-626, hashmap_linearprobe.hpp:430-515).
 *      Unlike the batch forms it is NOT followed by reserve(size()): the two differ after set_max_load_factor() lowered the
 *      threshold below the current size. */
kh_status kh_insert_one(kh_table* t, uint64_t key, uint32_t val, uint64_t* n_inserted /* 0 or 1 */);
/* update(k,v) applied in order to a batch: insert, or overwrite the existing value (last one wins)
 *      hashmap_robinhood.hpp:1274-1284 / hashmap_linearprobe.hpp:895-905 */
kh_status kh_update(kh_table* t, const void* keys, const void* vals, uint64_t n, kh_mem where, uint64_t* n_inserted);

/* ---- streamed insert: ONE insert(Iter,Iter) whose pairs arrive in pieces (the multi-GPU exchange delivers them peer by
 *      peer / chunk by chunk: khmxx::ialltoallv_and_modify, incremental_mxx.hpp:3437-3645, calls insert_no_estimate per
 *      block).  kh_insert_begin announces the exact total; every kh_insert_feed radix-partitions its piece at once and
 *      returns without synchronising (device pointers), so that work overlaps the next transfer; kh_insert_end de-duplicates
 *      and builds once.  The result equals kh_insert of the concatenated pieces in feed order (first value wins, same
 *      capacity rule).  reduce_plus != 0: kh_insert_reduce_plus semantics (vals may be NULL).  At most 16 feeds.  Between begin and
 *      end every other call that mutates the table or uses its workspace (insert, update, erase, rehash, reserve, clear, find,
 *      count, to_vector, displacement_histogram) returns KH_ERR_INVALID.  Host buffers (KH_MEM_HOST) may be reused as soon as
 *      kh_insert_feed returns; device buffers must stay valid until the work queued on the table's stream has consumed them
 *      (kh_insert_end synchronises). */
kh_status kh_insert_begin(kh_table* t, uint64_t n_total, int reduce_plus);
/* (same reference interface as kh_insert_begin: insert_no_estimate per received block, incremental_mxx.hpp:3437-3645)
 * flags: KH_INS_REDUCE_PLUS = kh_insert_begin's reduce_plus.  KH_INS_REPEATABLE: the caller keeps every piece it feeds (valid and
 *      unchanged) until kh_insert_end has returned and can feed them again.  The library may then partition the pieces without a
 *      histogram pass into slots they share (and without stream positions when a sample of the first piece shows no duplicate key);
 *      if that does not hold for the batch -- skewed or duplicated keys -- kh_insert_end returns KH_ERR_RETRY with the table
 *      unchanged, and the caller repeats begin (without the flag) / feed / end.  (The multi-GPU layer keeps its receive buffers.) */
#define KH_INS_REDUCE_PLUS 1u
#define KH_INS_REPEATABLE 2u
/* kh_insert_reduce semantics for the streamed form: a 2-bit field (bits 2-3) that holds the kh_reduce_op next to KH_INS_REDUCE_PLUS,
 *      which switches the reducer on.  KH_INS_REDUCE(op) builds the flags of any operation; KH_INS_REDUCE(KH_REDUCE_PLUS) is
 *      KH_INS_REDUCE_PLUS itself.  An operation field without KH_INS_REDUCE_PLUS is an unknown combination: KH_ERR_INVALID.  Feeds of a
 *      min / max / or insert need values (vals == NULL: KH_ERR_INVALID); KH_INS_REPEATABLE and kh_insert_abort keep their promises. */
#define KH_INS_REDUCE_OP_SHIFT 2
#define KH_INS_REDUCE_OP_MASK 12u
#define KH_INS_REDUCE(op) (KH_INS_REDUCE_PLUS | ((unsigned)(op) << KH_INS_REDUCE_OP_SHIFT))
#define KH_INS_REDUCE_MIN KH_INS_REDUCE(1)
#define KH_INS_REDUCE_MAX KH_INS_REDUCE(2)
#define KH_INS_REDUCE_OR KH_INS_REDUCE(3)
kh_status kh_insert_begin_ex(kh_table* t, uint64_t n_total, unsigned flags);
kh_status kh_insert_feed(kh_table* t, const void* keys /*[h|d] u64[n]*/, const void* vals /*[h|d] u32[n]*/, uint64_t n, kh_mem where);
kh_status kh_insert_end(kh_table* t, uint64_t* n_inserted);
/* gives up a streamed insert after kh_insert_begin: the pieces fed so far are dropped, nothing is inserted and the table is usable
 * again (the feeds only write workspace).  What the reference does when an exception leaves ialltoallv_and_modify's block loop
 * (incremental_mxx.hpp:3437-3645): the partially received batch is simply not inserted.  Synchronises the table's stream (queued
 * partition kernels may still read the caller's buffers).  No-op without a streamed insert in progress. */
kh_status kh_insert_abort(kh_table* t);

/* ---- reducer insert: the Reducer = std::plus form of the reference's batched table,
 *      hashmap_robinhood_offsets_reduction::insert(keys, T(1)) / insert(pairs) (robinhood_offset_hashmap_ptr.hpp:85-97,
 *      2787-2885) as used by dsc::counting_batched_robinhood_map (distributed_batched_robinhood_map.hpp:2542-2543,2633,2899):
 *      the value of a key becomes the (wrapping 32-bit) sum of the values of all its occurrences; vals == NULL means
 *      every occurrence contributes 1 (k-mer counting).  Results only are specified by the reference here (its own
 *      container sizes itself from a HyperLogLog estimate); capacity follows this table's doubling rule. */
kh_status kh_insert_reduce_plus(kh_table* t, const void* keys /*[h|d] u64[n]*/, const void* vals /*[h|d] u32[n] or NULL*/,
                                uint64_t n, kh_mem where, uint64_t* n_inserted);
/* ---- reducer insert with another Reducer: the reference's reduction maps call reduc(stored, incoming) for whatever functor they are
 *      instantiated with ("plus, max, etc.", robinhood_offset_hashmap_ptr.hpp:85-98, 1563-1565, 3058-3075).  Values are unsigned 32-bit;
 *      min and max compare them unsigned.  A key the table does not hold is inserted with the reduction of the values of all its
 *      occurrences in the batch (no identity element is involved); a key it holds gets op(stored, that reduction).  The key set, size,
 *      capacity and info bytes afterwards are exactly those of kh_insert_reduce_plus over the same keys: only the values differ.
 *      KH_REDUCE_PLUS is kh_insert_reduce_plus (vals == NULL: every occurrence contributes 1); for the other operations vals == NULL is
 *      KH_ERR_INVALID, and so is an unknown op.  min, max and or are commutative, associative and idempotent: the result does not
 *      depend on scheduling.  (ReplaceReducer, last value wins, is kh_insert followed by kh_update.) */
typedef enum { KH_REDUCE_PLUS = 0, KH_REDUCE_MIN = 1, KH_REDUCE_MAX = 2, KH_REDUCE_OR = 3 } kh_reduce_op;
kh_status kh_insert_reduce(kh_table* t, const void* keys /*[h|d] u64[n]*/, const void* vals /*[h|d] u32[n]; NULL with KH_REDUCE_PLUS only*/,
                           uint64_t n, kh_mem where, kh_reduce_op op, uint64_t* n_inserted);

/* ---- count(Iter,Iter): 0/1 per query in query order  hashmap_robinhood.hpp:1111-1160 / hashmap_linearprobe.hpp:639-688
 *      (the reference returns vector<size_t>; one byte per query here) */
kh_status kh_count(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint8_t* out01 /*[h|d] u8[n]*/);

/* ---- find: per-query form (value + found flag) and the reference's compacted form
 *      find(Iter,Iter) -> vector<pair> of hits in query order  hashmap_robinhood.hpp:1194-1268 / hashmap_linearprobe.hpp:816-889 */
kh_status kh_find(kh_table* t, const void* keys, uint64_t n, kh_mem where,
                  uint32_t* out_vals /*[h|d] u32[n], untouched on miss*/, uint8_t* out_found /*[h|d] u8[n]*/, uint64_t* n_found);
kh_status kh_find_compact(kh_table* t, const void* keys, uint64_t n, kh_mem where,
                          uint64_t* out_keys /*[h|d] u64[n]*/, uint32_t* out_vals /*[h|d] u32[n]*/, uint64_t* n_found);
kh_status kh_find_compact_pairs(kh_table* t, const void* keys, uint64_t n, kh_mem where,
                                void* out_pairs16 /*[h|d] 16 B x n*/, uint64_t* n_found);

/* ---- erase(Iter,Iter)  hashmap_robinhood.hpp:1430-1440 (never shrinks) / hashmap_linearprobe.hpp:1042-1051 (may shrink) */
kh_status kh_erase(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint64_t* n_erased);
/* erase(key) single-key form: also halves the table when size < min_load (:1421-1428 / :1032-1039).  The erase comes first: if
   the halved Robin Hood table cannot be laid out (home buckets merge past distance 127) the call returns KH_ERR_PROBE_OVERFLOW
   with the key ERASED (*n_erased = 1) and the capacity as it was; the table is consistent and usable. */
kh_status kh_erase_one(kh_table* t, uint64_t key, uint64_t* n_erased);

/* ---- iteration / parity exports (host buffers) */
kh_status kh_to_vector(kh_table* t, uint64_t* keys_host, uint32_t* vals_host, uint64_t* n_out); /* to_vector() :388, slot order */
kh_status kh_export_info(kh_table* t, uint8_t* out_host /* capacity bytes, reference encoding of the table's kind */);
kh_status kh_export_slots(kh_table* t, uint64_t* keys_host, uint32_t* vals_host /* capacity entries; empty slots unspecified */);
/* the table as it lies: capacity entries of 16 bytes {u64 key, u32 value, u32 info}; the low byte of `info` is the reference's
 * info byte of the table's kind (hashmap_robinhood.hpp:137-163 / hashmap_linearprobe.hpp:109-139), key and value of an empty slot are
 * unspecified.  What the reference exposes as `container` + `info_container` to its iterators (hashmap_robinhood.hpp:295-309); the
 * C++ shim probes such a snapshot on the host for loops of single-key const calls (find(key) / count(key), :1102,:1165). */
kh_status kh_export_raw_slots(kh_table* t, void* out_host /* capacity x 16 B */);
kh_status kh_displacement_histogram(kh_table* t, uint64_t out[128]); /* RH only: #slots per probe distance (REPROBE_STAT) */

/* ---- value-range operations: the elements whose 32-bit value v satisfies lo <= v <= hi (unsigned), found by ONE streaming pass over
 *      the slots instead of a kh_to_vector to the host.  The reference's batched maps take an output predicate over the stored
 *      (key, value) pair on count / find / erase (robinhood_offset_hashmap_ptr.hpp:1337-1407, 3484-3587;
 *      distributed_batched_robinhood_map.hpp:1202-1261, 2112-2428); a C ABI cannot take a functor, the closed value range is the
 *      predicate of k-mer counting (spectrum, abundance filter).  lo > hi is the empty range: nothing is selected or erased, KH_OK.
 *      Between kh_insert_begin and kh_insert_end all three return KH_ERR_INVALID.  Each synchronises the table's stream. */
/* out[b] = number of elements with value == b for b < nbins-1, out[nbins-1] = number with value >= nbins-1 (the bins sum to size());
 *      nbins 1..16384, anything else KH_ERR_INVALID */
kh_status kh_value_histogram(kh_table* t, uint32_t nbins, uint64_t* out_host /* u64[nbins] */);
/* the elements in the range, in slot order (the order of kh_to_vector), into host or device buffers as `where` says.  *n_out always
 *      receives the number of matches; out_keys == NULL: count only (out_vals == NULL: keys only).  More matches than cap_out:
 *      KH_ERR_INVALID, *n_out set, nothing written.  lo = 0, hi = UINT32_MAX with KH_MEM_DEVICE: to_vector() into device memory. */
kh_status kh_select_values(kh_table* t, uint32_t lo, uint32_t hi, kh_mem where, uint64_t* out_keys /*[h|d] u64[cap_out] or NULL*/,
                           uint32_t* out_vals /*[h|d] u32[cap_out] or NULL*/, uint64_t cap_out, uint64_t* n_out);
/* erases every element in the range: the table afterwards equals the table after kh_erase of exactly those keys (size, capacity,
 *      info array, contents, and kh_erase's tail: RH reserve(size()) only, LP the shrinking rehash when size < min_load).  RH: if
 *      the re-layout fails the table is unchanged. */
kh_status kh_erase_values(kh_table* t, uint32_t lo, uint32_t hi, uint64_t* n_erased);

/* ---- batched hashing: Hash::operator()(Key const*, count, out)  murmurhash3_64_avx.hpp:1584-1597, hash_new.hpp:1035-1056 */
kh_status kh_hash_batch(kh_hash hash, uint64_t seed, const void* keys, uint64_t n, kh_mem where,
                        uint64_t* out /*[h|d]*/, int device, void* hip_stream);
/* TransformedHash::operator()(Key const*, count, out)  hash_new.hpp:1035-1056: out[i] = hash(pre_transform(keys[i])) */
kh_status kh_hash_batch_transformed(kh_hash hash, uint64_t seed, kh_key_transform xf, uint32_t k, const void* keys, uint64_t n,
                                    kh_mem where, uint64_t* out /*[h|d]*/, int device, void* hip_stream);

/* ---- key-space sharding for the multi-GPU layer: rank = hash(key, seed) & (p-1) (p power of two) or % p
 *      (distributed_batched_robinhood_map.hpp:513-534,632-741 assign_count_permute).  Device buffers only.
 *      out_* receive the pairs grouped by destination rank (rank 0 first, input order kept inside a rank);
 *      counts_host[p] receives the per-rank element counts.  out_keys_dev == NULL: count only (nothing is permuted). */
kh_status kh_shard_permute(kh_hash hash, uint64_t seed, uint32_t nranks,
                           const uint64_t* keys_dev, const uint32_t* vals_dev /* may be NULL */, uint64_t n,
                           uint64_t* out_keys_dev /* may be NULL */, uint32_t* out_vals_dev /* may be NULL */,
                           uint64_t* counts_host, int device, void* hip_stream);
/* the same with the distributed map's TransformedHash (rank = hash(pre_transform(key)) mod p: both strands of a k-mer go to one rank) */
kh_status kh_shard_permute_transformed(kh_hash hash, uint64_t seed, kh_key_transform xf, uint32_t k, uint32_t nranks,
                                       const uint64_t* keys_dev, const uint32_t* vals_dev, uint64_t n,
                                       uint64_t* out_keys_dev, uint32_t* out_vals_dev, uint64_t* counts_host, int device, void* hip_stream);

/* ---- a batch that will be exchanged in `pieces` pieces (the pipelined insert, khmxx::ialltoallv_and_modify incremental_mxx.hpp:3437-3645):
 *      the counting half of assign_count_permute (distributed_batched_robinhood_map.hpp:632-741) done ONCE -- one count sweep + scan +
 *      host synchronisation for the whole batch.  bounds_host[pieces+1] receives the piece boundaries (multiples of 4096 pairs, the last one = n),
 *      counts_host[pieces][nranks] the destination counts of every piece; kh_shard_plan_permute then permutes piece i (pairs
 *      [bounds[i], bounds[i+1]) of the SAME keys/vals arrays, unchanged since the plan was made) into out_* grouped by rank, input
 *      order kept, without counting again and without synchronising.  nranks <= 8.  Same result as kh_shard_permute on the piece. */
typedef struct kh_shard_plan kh_shard_plan;
kh_status kh_shard_plan_create(kh_shard_plan** out, kh_hash hash, uint64_t seed, kh_key_transform xf, uint32_t k, uint32_t nranks,
                               const uint64_t* keys_dev, uint64_t n, uint32_t pieces, uint64_t* counts_host, uint64_t* bounds_host,
                               int device, void* hip_stream);
kh_status kh_shard_plan_permute(kh_shard_plan* plan, uint32_t piece, const uint64_t* keys_dev, const uint32_t* vals_dev /* may be NULL */,
                                uint64_t* out_keys_dev, uint32_t* out_vals_dev, void* hip_stream);
/* (same reference interface: the permutation half of assign_count_permute, distributed_batched_robinhood_map.hpp:632-741, as the
 * pipelined queries khmxx::ialltoallv_and_query_one_to_one use it, incremental_mxx.hpp:4403-4669)  piece i written to ITS PLACE in the
 * layout of the whole batch grouped by rank -- out_* have room for all n pairs and end up, once every piece has been permuted, equal to
 * kh_shard_permute's output; the part of rank r that piece i contributes is contiguous: it starts at offsets[r][i] and ends at
 * offsets[r][i + 1] (kh_shard_plan_offsets: [nranks][pieces + 1] positions in that layout). */
kh_status kh_shard_plan_permute_global(kh_shard_plan* plan, uint32_t piece, const uint64_t* keys_dev, const uint32_t* vals_dev /* may be NULL */,
                                       uint64_t* out_keys_dev, uint32_t* out_vals_dev, void* hip_stream);
kh_status kh_shard_plan_offsets(const kh_shard_plan* plan, uint64_t* offsets_host /* [nranks][pieces+1] */);
/* Stream-ordered: destroy may be called as soon as the last kh_shard_plan_permute / _permute_global call has RETURNED, with the
 * permutations still queued; the plan's device block returns to the library's pool only after every permutation queued from the plan has run
 * (a host function queued behind them on their streams; a stream that refuses it is waited for).  A plan that was never permuted, or
 * with n == 0, is freed at once.  The handle itself is invalid from the call on.  Permutations captured into a graph read the block
 * at every replay: there the block is freed at once and nothing is queued, so destroy such a plan after the last replay.  NULL: no-op. */
void kh_shard_plan_destroy(kh_shard_plan* plan);

/* ---- k-mer generation front end (BenchmarkKmerCounter.cpp:1655-1706 reads sequences through kmerind's
 *      KmerParser, which is not part of the reference tree: PARITY UNPINNED, the definition below is this library's):
 *      every window of k valid bases (ACGT, either case) of `seq` yields one 2-bit packed k-mer (first base most
 *      significant, A=0 C=1 G=2 T=3), in sequence order; any other byte ends the run (pass read/sequence lines separated
 *      by '\n').  canonical != 0: min(k-mer, reverse complement).  out_kmers needs room for n entries. */
kh_status kh_kmers_from_sequence(const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where,
                                 uint64_t* out_kmers /*[h|d]*/, uint64_t* n_out, int device, void* hip_stream);
/* the same over raw FASTQ text (BenchmarkKmerCounter.cpp:1476-1560 reads FASTQ through kmerind's FASTQParser, absent: PARITY
 *      UNPINNED): records of 4 lines (@id, sequence, +, quality) starting at byte 0 of `text`; only the sequence lines
 *      (line number 1 mod 4, counted by '\n') yield k-mers, a k-mer never spans two reads.  Pass whole records. */
kh_status kh_kmers_from_fastq(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where,
                              uint64_t* out_kmers /*[h|d]*/, uint64_t* n_out, int device, void* hip_stream);

/* the same k-mers, in the same order and with the same n_out, each with the byte offset of the first base of its window in the buffer
 *      passed: out_pos[i] belongs to out_kmers[i] (for FASTQ an offset into the raw text, not into a read).  canonical != 0: the offset
 *      is the window's; which strand the canonical form came from is not recorded here: kh_stamp_strand recovers it from (text, offsets).
 *      Positions are 32-bit: n >= 2^32 is KH_ERR_INVALID before anything is allocated or read.  out_pos needs room for n entries. */
kh_status kh_kmers_from_sequence_pos(const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where,
                                     uint64_t* out_kmers /*[h|d]*/, uint32_t* out_pos /*[h|d]*/, uint64_t* n_out, int device, void* hip_stream);
kh_status kh_kmers_from_fastq_pos(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where,
                                  uint64_t* out_kmers /*[h|d]*/, uint32_t* out_pos /*[h|d]*/, uint64_t* n_out, int device, void* hip_stream);
/* ---- k-mer position index: ALL occurrences per k-mer (the reference's driver offers PositionIndex<MapType> over a multimap next to
 *      CountIndex, BenchmarkKmerIndex.cpp:342-449; the multimap is kmerind's and absent from the reference tree: the contract below is
 *      this library's).  An index of 64-bit keys (k <= 32) on one GPU: built from a batch of (key, position) pairs, queried, and changed
 *      batch by batch (kh_index_append*, kh_index_erase, kh_index_erase_counts below).  State: one Robin Hood table owned by the index plus offsets u32[size + 1] and positions u32[total] in device memory.
 *      After a build the table's value of a key is its RANK among the live slots in slot order (0..size-1) and positions[offsets[rank]
 *      .. offsets[rank + 1]) are the positions of that key: a lookup reads one slot and two adjacent offsets words.
 *      kh_index_build: the index must be empty (else KH_ERR_INVALID; kh_index_clear empties it); n >= 2^32: KH_ERR_INVALID before
 *      anything is touched; n == 0: KH_OK, the index stays empty.  Afterwards key set, size, capacity, info bytes and slot order of the
 *      table are those of a fresh Robin Hood table (capacity 128) with the same hash, seed (no key transform) and load factors after
 *      kh_insert_reduce_plus(keys, NULL, n) -- except that the keys which share a HOME BUCKET, whose order among themselves that insert
 *      leaves to scheduling, stand in ascending key order; offsets[0] = 0, offsets[size] = n.  THE POSITIONS OF ONE KEY ASCEND NUMERICALLY WHATEVER
 *      THE ORDER OF THE INPUT PAIRS: the result is a function of the multiset of pairs, hash, seed and load factors only (two builds
 *      export identical bytes).  Duplicate pairs are kept.  On any failure (KH_ERR_PROBE_OVERFLOW, a refused batch, KH_ERR_NOMEM, ...)
 *      the index is left empty.  Device pairs must stay valid until the call returns; every call synchronises the index's stream.
 *      kh_index_build_from_sequence / _from_fastq: kh_kmers_from_sequence_pos / _fastq_pos and the build, on device buffers (host text
 *      is staged once; k-mers and positions never visit the host).
 *      kh_index_export: keys in slot order (the order of kh_to_vector), offsets and positions, into host buffers (any may be NULL).
 *      The linear-probe layout is not supported; a strand bit per occurrence: kh_index_set_stranded below; 16-byte keys (k <= 64) are kh_wide_index_* below. */
typedef struct kh_index kh_index;
kh_status kh_index_create(kh_index** out, kh_hash hash, uint64_t seed, float min_lf, float max_lf, int device);
kh_status kh_index_destroy(kh_index* x);
/* the index's work is issued on this stream; like kh_set_stream it waits for the old stream before it switches, so earlier calls stay
 * ordered before later ones.  Every batch call of an index synchronises the stream before it returns. */
kh_status kh_index_set_stream(kh_index* x, void* hip_stream);
const char* kh_index_last_error(const kh_index* x);
kh_status kh_index_clear(kh_index* x);
kh_status kh_index_build(kh_index* x, const void* keys /*[h|d] u64[n]*/, const void* pos /*[h|d] u32[n]*/, uint64_t n, kh_mem where);
kh_status kh_index_build_from_sequence(kh_index* x, const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where);
kh_status kh_index_build_from_fastq(kh_index* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where);
kh_status kh_index_size(const kh_index* x, uint64_t* distinct_keys);
kh_status kh_index_total(const kh_index* x, uint64_t* n_positions);
kh_status kh_index_capacity(const kh_index* x, uint64_t* buckets);
kh_status kh_index_export(kh_index* x, uint64_t* keys_host /*[size]*/, uint32_t* offsets_host /*[size+1]*/, uint32_t* positions_host /*[total]*/);
/* ---- changing a built index.  kh_index_append adds n pairs to an index in ANY state; on an empty index it is kh_index_build (the same
 *      kernels, the same bytes).  After build(A1), append(A2), ..., append(Am): count, find and export are those of the index of the
 *      concatenated pairs -- every key's positions ascend, duplicate pairs are kept -- and key set, size, capacity and info bytes of the
 *      table are those of a fresh counting table after kh_insert_reduce_plus(A1), ..., kh_insert_reduce_plus(Am) in that order, the keys
 *      of one home bucket in ascending key order.  The export is a function of the SEQUENCE OF BATCH MULTISETS: permuting the pairs
 *      inside a batch changes no byte, and where that table's capacity equals the capacity of one insert of the concatenation the export
 *      is byte-identical to the one-shot build.
 *      kh_index_append_from_sequence / _from_fastq: the windows of kh_kmers_from_sequence_pos / _fastq_pos with pos_base added to every
 *      window position on the device, so that several texts share one coordinate space.
 *      kh_index_erase removes every occurrence of the given keys (misses and repeated keys are harmless); kh_index_erase_counts removes
 *      every key whose number of occurrences lies in the closed range [lo, hi] (the range language of kh_erase_values; lo > hi is the
 *      empty range: KH_OK, nothing erased).  *n_keys_erased: distinct keys removed, *n_pos_erased: positions removed (either may be
 *      NULL).  Afterwards the index is that of the pairs whose key survives, and the table equals the counting twin after kh_erase of
 *      the same keys (size, capacity, info bytes; home-bucket runs in key order).  Erasing every key leaves a usable empty index ON THE
 *      TABLE AS kh_erase LEFT IT: it keeps its capacity, like a cleared table (kh_clear), unlike kh_index_clear, which goes back to a
 *      fresh table of capacity 128 -- a later append or build lays out like the twin with the same history.
 *      Refused with KH_ERR_INVALID before anything is touched (the index unchanged): a null argument, total + n >= 2^32,
 *      pos_base + n > 2^32 (a window position would wrap), k out of range.  A failure after the table was touched
 *      (KH_ERR_PROBE_OVERFLOW, KH_ERR_NOMEM, a HIP error) leaves the index EMPTY as a failed build does (fresh table); the error text
 *      survives.  Every call synchronises the index's stream.  Peak device memory of an append or erase: the old and the new positions
 *      (and offsets) arrays side by side, the batch (for an append with 4 B of zero values per pair during the table insert), and for an
 *      append the sort scratch of the build (4 B per position). */
kh_status kh_index_append(kh_index* x, const void* keys /*[h|d] u64[n]*/, const void* pos /*[h|d] u32[n]*/, uint64_t n, kh_mem where);
kh_status kh_index_append_from_sequence(kh_index* x, const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where, uint32_t pos_base);
kh_status kh_index_append_from_fastq(kh_index* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, int canonical, kh_mem where, uint32_t pos_base);
kh_status kh_index_erase(kh_index* x, const void* keys /*[h|d] u64[n]*/, uint64_t n, kh_mem where, uint64_t* n_keys_erased, uint64_t* n_pos_erased);
kh_status kh_index_erase_counts(kh_index* x, uint32_t lo, uint32_t hi, uint64_t* n_keys_erased, uint64_t* n_pos_erased);
/* occurrences of every query key, 0 on a miss */
kh_status kh_index_count(kh_index* x, const void* keys /*[h|d] u64[n]*/, uint64_t n, kh_mem where, uint32_t* out_counts /*[h|d] u32[n]*/);
/* a CSR in query order: out_offsets = exclusive scan of the counts, out_offsets[n] = *n_out = the number of positions; the positions
 *      of query i are out_pos[out_offsets[i] .. out_offsets[i + 1]), ascending; a repeated query key repeats its positions.
 *      out_pos == NULL: out_offsets and *n_out only.  More positions than cap_out: KH_ERR_INVALID, *n_out set (out_offsets too),
 *      nothing written to out_pos (the convention of kh_select_values). */
kh_status kh_index_find(kh_index* x, const void* keys /*[h|d] u64[n]*/, uint64_t n, kh_mem where,
                        uint64_t* out_offsets /*[h|d] u64[n+1]*/, uint32_t* out_pos /*[h|d] u32[cap_out] or NULL*/,
                        uint64_t cap_out, uint64_t* n_out);
/* per-kernel timing of the index's own table (kh_profile_enable / kh_profile_dump): the counting insert's kernels and k_index_* */
kh_status kh_index_profile_enable(kh_index* x, int on);
kh_status kh_index_profile_dump(kh_index* x, char* buf, uint64_t cap);

/* ---- HyperLogLog cardinality estimator: fsc::hyperloglog64<T, Hash, precision> (hyperloglog64.hpp:142-475),
 *      64-bit hash values: register = top `precision` bits after dropping `ignore_msb` bits, rank = leading zeros + 1
 *      (:175-188); estimate() = harmonic mean with the linear-counting branch below 5m/2 (:201-236).  Registers are
 *      bit-exact with the reference; the estimate is computed on the host in the reference's operation order. */
typedef struct kh_hll kh_hll;
kh_status kh_hll_create(kh_hll** out, uint32_t precision /*12*/, uint32_t ignore_msb /*0*/, kh_hash hash, uint64_t seed, int device);
kh_status kh_hll_destroy(kh_hll* h);
/* the estimator's work is issued on this stream; like kh_set_stream it waits for the old stream before it switches, so an update queued
 * under one stream is seen by kh_hll_registers / _estimate / _clear / a further update under the next, and kh_hll_destroy never frees
 * registers a queued kernel still writes.  kh_hll_merge(h, other) runs on h's stream and first waits for other's stream when the two
 * differ; the read of other's registers is only queued: other must not be updated, cleared or destroyed until h's stream has run the
 * merge (kh_hll_registers(h) waits for it).  Updates from device memory, merge, clear and the text passes with n_kmers == NULL return without synchronising: their
 * input must stay valid until the estimator's stream has run them (kh_hll_registers and kh_hll_estimate synchronise). */
kh_status kh_hll_set_stream(kh_hll* h, void* hip_stream);
kh_status kh_hll_update(kh_hll* h, const void* keys /*[h|d] u64[n]*/, uint64_t n, kh_mem where);               /* update(vals,count) :357 */
kh_status kh_hll_update_via_hashval(kh_hll* h, const void* hashes /*[h|d] u64[n]*/, uint64_t n, kh_mem where); /* :449-455 */
kh_status kh_hll_merge(kh_hll* h, const kh_hll* other);   /* :463 */
kh_status kh_hll_clear(kh_hll* h);                        /* :467 */
kh_status kh_hll_registers(kh_hll* h, uint8_t* out_host /* 2^precision bytes */);
kh_status kh_hll_estimate(kh_hll* h, double* out);       /* :459 */
/* internal_estimate (:201-236) on 2^precision host registers: what estimate_global (:482-484) applies to the registers merged over all
 * ranks (merge_distributed :477-479 = an all-reduce(max) of the registers, done by the caller's communication layer).  Host only. */
kh_status kh_hll_estimate_registers(const uint8_t* registers_host, uint32_t precision, double* out);

/* ---- wide keys: a Robin Hood table of 16-byte keys with 32-bit values (k-mers up to k = 64).  A wide key is {uint64_t w0, uint64_t w1},
 *      w0 at offset 0: the memory image of a 16-byte POD key such as kmerind's Kmer<63, DNA, uint64_t>, and the hashes read these 16
 *      bytes in this order (KH_HASH_IDENTITY: w0; murmur3: MurmurHash3_x86_128 / _x64_128 over 16 bytes; farm: Hash64WithSeed(key, 16,
 *      seed), parity unpinned as for 8 bytes).  A k-mer with k <= 64 is the 128-bit integer V (first base most significant, A0 C1 G2 T3,
 *      as for 64-bit k-mers) stored as w0 = V mod 2^64, w1 = V >> 64 -- for k <= 32, w0 is the 64-bit k-mer and w1 = 0; its canonical
 *      form is min(V, revcomp_k(V)) as 128-bit unsigned integers.  kmerind's own Kmer bit layout is not part of the reference tree:
 *      PARITY UNPINNED for the packing.  Batches of keys are u64[2n] ([h|d] as elsewhere).  The table follows the 64-bit Robin Hood
 *      table rule for rule (float load thresholds, one doubling per insert() call while size >= max_load, the trailing reserve(size()),
 *      batch erase never shrinks, first value wins, std::plus wraps at 32 bits, KH_ERR_PROBE_OVERFLOW leaves the table unchanged);
 *      its info array (kh_wide_export_info) is the canonical Robin Hood layout of the key set at the capacity.  A distinct handle type:
 *      a kh_wtable passed to a kh_table entry point does not compile.
 *      ALIGNMENT: A DEVICE ARRAY OF 16-BYTE KEYS MUST BE 16-BYTE ALIGNED wherever a key is moved as one 16-byte access.  Every entry point
 *      that READS such an array with KH_MEM_DEVICE and n > 0 -- kh_wide_insert / _insert_reduce_plus / _insert_reduce / _insert_feed,
 *      kh_wide_count / _find / _find_compact / _erase, kh_wide_hash_batch, kh_wide_shard_permute, kh_hll_update_wide,
 *      kh_wide_syncmer_mask and kh_wide_index_build / _append / _erase / _count / _find -- and every one that WRITES one with a 16-byte
 *      store per key -- out_keys_dev of kh_wide_shard_permute, out_kmers of kh_kmers128_from_sequence / _from_fastq and their _pos
 *      forms and of kh_syncmers128_from_sequence / _from_fastq -- returns KH_ERR_INVALID otherwise, before anything is launched: the
 *      handle, its table or registers, *n_out (0) and every output array are untouched (a streamed insert stays open with nothing
 *      fed).  Host arrays may have any alignment, they are staged.  Only out_keys of kh_wide_find_compact and of kh_wide_select_values
 *      are written as two 64-bit words per key: 8-byte alignment is enough there. */
typedef struct kh_wtable kh_wtable;
kh_status kh_wide_create(kh_wtable** out, kh_kind kind /* KH_KIND_LINEARPROBE: KH_ERR_UNSUPPORTED */, kh_hash hash, uint64_t seed,
                         uint64_t capacity, float min_load_factor, float max_load_factor, int device);
kh_status kh_wide_destroy(kh_wtable* t);
kh_status kh_wide_set_stream(kh_wtable* t, void* hip_stream);
const char* kh_wide_last_error(const kh_wtable* t);
kh_status kh_wide_size(const kh_wtable* t, uint64_t* out);
kh_status kh_wide_capacity(const kh_wtable* t, uint64_t* out);
kh_status kh_wide_get_load_factors(const kh_wtable* t, float* min_lf, float* max_lf, float* current);
kh_status kh_wide_set_min_load_factor(kh_wtable* t, float f);
kh_status kh_wide_set_max_load_factor(kh_wtable* t, float f);
kh_status kh_wide_clear(kh_wtable* t);
kh_status kh_wide_reserve(kh_wtable* t, uint64_t n);
kh_status kh_wide_rehash(kh_wtable* t, uint64_t buckets);
kh_status kh_wide_insert(kh_wtable* t, const void* keys /*[h|d] u64[2n]*/, const void* vals /*[h|d] u32[n]*/, uint64_t n, kh_mem where,
                         uint64_t* n_inserted);
kh_status kh_wide_insert_reduce_plus(kh_wtable* t, const void* keys /*[h|d] u64[2n]*/, const void* vals /*[h|d] u32[n] or NULL*/, uint64_t n,
                                     kh_mem where, uint64_t* n_inserted);
/* kh_insert_reduce for 16-byte keys */
kh_status kh_wide_insert_reduce(kh_wtable* t, const void* keys /*[h|d] u64[2n]*/, const void* vals /*[h|d] u32[n]; NULL with KH_REDUCE_PLUS only*/,
                                uint64_t n, kh_mem where, kh_reduce_op op, uint64_t* n_inserted);
kh_status kh_wide_count(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint8_t* out01 /*[h|d] u8[n]*/);
kh_status kh_wide_find(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint32_t* out_vals /*[h|d] u32[n], untouched on miss*/,
                       uint8_t* out_found /*[h|d] u8[n]*/, uint64_t* n_found);
kh_status kh_wide_find_compact(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint64_t* out_keys /*[h|d] u64[2n]*/,
                               uint32_t* out_vals /*[h|d] u32[n]*/, uint64_t* n_found);
kh_status kh_wide_erase(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint64_t* n_erased);
kh_status kh_wide_to_vector(kh_wtable* t, uint64_t* keys_host /* u64[2 size] */, uint32_t* vals_host, uint64_t* n_out);
kh_status kh_wide_export_info(kh_wtable* t, uint8_t* out_host /* capacity bytes */);
kh_status kh_wide_displacement_histogram(kh_wtable* t, uint64_t out[128]);
/* kh_value_histogram / kh_select_values / kh_erase_values of a wide table; selected keys are u64[2 n] */
kh_status kh_wide_value_histogram(kh_wtable* t, uint32_t nbins, uint64_t* out_host /* u64[nbins] */);
kh_status kh_wide_select_values(kh_wtable* t, uint32_t lo, uint32_t hi, kh_mem where, uint64_t* out_keys /*[h|d] u64[2 cap_out] or NULL*/,
                                uint32_t* out_vals /*[h|d] u32[cap_out] or NULL*/, uint64_t cap_out, uint64_t* n_out);
kh_status kh_wide_erase_values(kh_wtable* t, uint32_t lo, uint32_t hi, uint64_t* n_erased);
/* ---- streamed insert of a wide table: the contract written above kh_insert_begin, for 16-byte keys.  The result equals ONE
 *      kh_wide_insert (KH_INS_REDUCE_PLUS: kh_wide_insert_reduce_plus, vals may then be NULL) of the pieces concatenated in feed order:
 *      first value wins between pieces, same capacity rule, same trailing reserve(size()).  A feed of device memory only queues the
 *      counting half of the partition on its piece and returns without synchronising; DEVICE BUFFERS MUST STAY VALID AND UNCHANGED
 *      UNTIL kh_wide_insert_end (or _abort) RETURNS -- they are read again there.  Host buffers are copied and may be reused as soon
 *      as the feed returns.  At most 16 non-empty feeds (KH_ERR_UNSUPPORTED beyond, whatever the state of the table).  Between begin and end every other call that
 *      mutates the table or uses its workspace returns KH_ERR_INVALID, and so do a feed beyond n_total, an end before n_total pairs
 *      were fed (which also closes the streamed insert, nothing inserted) and feed / end without begin.  kh_wide_insert_abort drops the
 *      pieces and leaves the table untouched and usable; it synchronises the table's stream.  KH_INS_REPEATABLE is accepted and changes
 *      nothing: the wide partition is exact (count, scan, scatter), so A WIDE TABLE NEVER RETURNS KH_ERR_RETRY. */
kh_status kh_wide_insert_begin_ex(kh_wtable* t, uint64_t n_total, unsigned flags /* KH_INS_REDUCE_PLUS or KH_INS_REDUCE(op) | KH_INS_REPEATABLE */);
kh_status kh_wide_insert_feed(kh_wtable* t, const void* keys /*[h|d] u64[2n]*/, const void* vals /*[h|d] u32[n] or NULL*/, uint64_t n,
                              kh_mem where);
kh_status kh_wide_insert_end(kh_wtable* t, uint64_t* n_inserted);
kh_status kh_wide_insert_abort(kh_wtable* t);
/* kh_shard_permute for 16-byte keys: rank = hash of the 16 bytes (what kh_wide_hash_batch computes) & (nranks-1), or % nranks when
 *      nranks is not a power of two; pairs grouped by destination rank, rank 0 first, INPUT ORDER KEPT inside a rank.  Device buffers
 *      only; nranks 1..64; out_keys_dev == NULL: count only; n == 0: counts of 0.  keys_dev and out_keys_dev: the alignment rule of the wide keys
 *      (above kh_wide_create). */
kh_status kh_wide_shard_permute(kh_hash hash, uint64_t seed, uint32_t nranks,
                                const uint64_t* keys_dev /* u64[2n] */, const uint32_t* vals_dev /* may be NULL */, uint64_t n,
                                uint64_t* out_keys_dev /* u64[2n]; NULL = count only */, uint32_t* out_vals_dev,
                                uint64_t* counts_host, int device, void* hip_stream);
/* out[i] = hash of the 16-byte key i */
kh_status kh_wide_hash_batch(kh_hash hash, uint64_t seed, const void* keys /*[h|d] u64[2n]*/, uint64_t n, kh_mem where,
                             uint64_t* out /*[h|d]*/, int device, void* hip_stream);
/* kh_kmers_from_sequence / kh_kmers_from_fastq for k = 1..64: 16-byte k-mers {w0, w1} in order; out_kmers needs room for 2n words */
kh_status kh_kmers128_from_sequence(const void* seq, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where,
                                    uint64_t* out_kmers /*[h|d] u64[2n]*/, uint64_t* n_out, int device, void* hip_stream);
kh_status kh_kmers128_from_fastq(const void* text, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where,
                                 uint64_t* out_kmers /*[h|d] u64[2n]*/, uint64_t* n_out, int device, void* hip_stream);

/* ---- HyperLogLog for every k-mer length: updates from 16-byte keys and straight from text (the reference sizes its counting table from
 *      such an estimate before it inserts, robinhood_offset_hashmap_ptr.hpp:2484-2535; BenchmarkKmerCounter.cpp:1508-1590 estimates per
 *      file batch, before any k-mer buffer exists).  Registers live in hash-value space: one estimator may be fed by any mix of these
 *      calls, kh_hll_update and kh_hll_update_via_hashval.  Whether 8-byte and 16-byte keys belong in ONE estimate is the caller's
 *      business: the same k-mer hashes differently at the two widths.
 *      kh_hll_update_wide: the registers afterwards equal those after kh_hll_update_via_hashval of kh_wide_hash_batch(keys) with the
 *      estimator's hash and seed.  Device keys: the alignment rule of the wide keys (above kh_wide_create).
 *      kh_hll_update_from_sequence / _from_fastq: ONE pass text -> windows -> canonical form -> hash -> registers, 1 byte read per base
 *      and no k-mer written.  The registers afterwards equal those after kh_hll_update of kh_kmers_from_sequence / _from_fastq (k <= 32:
 *      the 8-byte k-mer is hashed) or kh_hll_update_wide of kh_kmers128_from_sequence / _from_fastq (k > 32: the 16-byte k-mer {w0, w1}),
 *      for the same text, k and canonical flag; *n_kmers receives the number of valid windows, the n_out of those front ends.  Text at
 *      any byte alignment; FASTQ text as for kh_kmers_from_fastq (whole 4-line records).
 *      All three: work is issued on the estimator's stream (kh_hll_set_stream).  n_kmers == NULL and device input: the call queues its
 *      work and returns without synchronising (the text must stay valid until that work has run); n_kmers != NULL, or host input: it
 *      synchronises.  KH_ERR_INVALID: a NULL handle, k outside 1..64, a NULL input with n > 0.  n == 0 (and a text shorter than k):
 *      KH_OK, registers unchanged, *n_kmers = 0. */
kh_status kh_hll_update_wide(kh_hll* h, const void* keys /*[h|d] u64[2n]*/, uint64_t n, kh_mem where);
kh_status kh_hll_update_from_sequence(kh_hll* h, const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/,
                                      int canonical, kh_mem where, uint64_t* n_kmers /* may be NULL */);
kh_status kh_hll_update_from_fastq(kh_hll* h, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/,
                                   int canonical, kh_mem where, uint64_t* n_kmers /* may be NULL */);

/* ---- measurement hooks: per-kernel HIP-event timing on the table's stream (bench.py roofline) */
kh_status kh_profile_enable(kh_table* t, int on);
kh_status kh_profile_reset(kh_table* t);
/* total ms and launch count of kernels whose name starts with `prefix` since the last reset */
kh_status kh_profile_query(kh_table* t, const char* prefix, double* total_ms, uint64_t* launches);
/* writes up to `cap` bytes of "name launches total_ms\n" lines */
kh_status kh_profile_dump(kh_table* t, char* buf, uint64_t cap);

/* ---- the position index over 16-byte keys (k-mers with k <= 64): kh_index_* word for word with a key of two 64-bit words {w0, w1}
 *      (keys u64[2n], as kh_wide_* takes them), on the wide Robin Hood table.  Built from an empty index; duplicate pairs
 *      kept; the positions of a key ascend; kh_wide_index_find returns a CSR in query order whose total is known before anything is
 *      written (too small a cap_out: KH_ERR_INVALID, the output buffers untouched); a failed build leaves the index empty; n >= 2^32 is
 *      refused; without a GPU kh_wide_index_create returns KH_ERR_HIP and a null handle.  After a build key set, size, capacity and info
 *      bytes of the table are those of a fresh kh_wide_create table (capacity 128, same hash, seed and load factors) after
 *      kh_wide_insert_reduce_plus(keys, NULL, n); the slot order is that table's up to the order of the keys that share a HOME BUCKET,
 *      which stand in ascending order of the 128-bit value (w1 << 64) | w0 -- so the export depends on the multiset of pairs alone.
 *      kh_wide_index_build_from_sequence / _from_fastq: kh_kmers128_from_sequence_pos / _fastq_pos and the build, k = 1..64.
 *      kh_wide_index_export: keys_host u64[2 size] in slot order (the order of kh_wide_to_vector).
 *      kh_wide_index_append* / _erase / _erase_counts: the contract of kh_index_append* / kh_index_erase / kh_index_erase_counts (twin:
 *      kh_wide_insert_reduce_plus batch by batch, kh_wide_erase), keys u64[2n], k = 1..64.
 *      Not supported: read-id decoding, 64-bit positions.  (A strand bit per occurrence: kh_wide_index_set_stranded.) */
typedef struct kh_windex kh_windex;
kh_status kh_wide_index_create(kh_windex** out, kh_hash hash, uint64_t seed, float min_lf, float max_lf, int device);
kh_status kh_wide_index_destroy(kh_windex* x);
kh_status kh_wide_index_set_stream(kh_windex* x, void* hip_stream);
const char* kh_wide_index_last_error(const kh_windex* x);
kh_status kh_wide_index_clear(kh_windex* x);
kh_status kh_wide_index_build(kh_windex* x, const void* keys /*[h|d] u64[2n]*/, const void* pos /*[h|d] u32[n]*/, uint64_t n, kh_mem where);
kh_status kh_wide_index_build_from_sequence(kh_windex* x, const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where);
kh_status kh_wide_index_build_from_fastq(kh_windex* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where);
kh_status kh_wide_index_append(kh_windex* x, const void* keys /*[h|d] u64[2n]*/, const void* pos /*[h|d] u32[n]*/, uint64_t n, kh_mem where);
kh_status kh_wide_index_append_from_sequence(kh_windex* x, const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where, uint32_t pos_base);
kh_status kh_wide_index_append_from_fastq(kh_windex* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where, uint32_t pos_base);
kh_status kh_wide_index_erase(kh_windex* x, const void* keys /*[h|d] u64[2n]*/, uint64_t n, kh_mem where, uint64_t* n_keys_erased, uint64_t* n_pos_erased);
kh_status kh_wide_index_erase_counts(kh_windex* x, uint32_t lo, uint32_t hi, uint64_t* n_keys_erased, uint64_t* n_pos_erased);
kh_status kh_wide_index_size(const kh_windex* x, uint64_t* distinct_keys);
kh_status kh_wide_index_total(const kh_windex* x, uint64_t* n_positions);
kh_status kh_wide_index_capacity(const kh_windex* x, uint64_t* buckets);
kh_status kh_wide_index_export(kh_windex* x, uint64_t* keys_host /*[2*size]*/, uint32_t* offsets_host /*[size+1]*/, uint32_t* positions_host /*[total]*/);
/* the RH info byte of every bucket of the index's table (kh_wide_export_info of it; out_host u8[capacity]): equal to the counting twin's */
kh_status kh_wide_index_export_info(kh_windex* x, uint8_t* out_host);
kh_status kh_wide_index_count(kh_windex* x, const void* keys /*[h|d] u64[2n]*/, uint64_t n, kh_mem where, uint32_t* out_counts /*[h|d] u32[n]*/);
kh_status kh_wide_index_find(kh_windex* x, const void* keys /*[h|d] u64[2n]*/, uint64_t n, kh_mem where,
                             uint64_t* out_offsets /*[h|d] u64[n+1]*/, uint32_t* out_pos /*[h|d] u32[cap_out] or NULL*/,
                             uint64_t cap_out, uint64_t* n_out);
kh_status kh_wide_index_profile_enable(kh_windex* x, int on);
kh_status kh_wide_index_profile_dump(kh_windex* x, char* buf, uint64_t cap);

/* kh_kmers_from_sequence_pos / _fastq_pos for 16-byte k-mers, k = 1..64: out_kmers u64[2n] ({w0, w1} per k-mer, the windows and the order of
 *      kh_kmers128_from_sequence / _fastq), out_pos[i] the byte offset of the first base of the window of k-mer i */
kh_status kh_kmers128_from_sequence_pos(const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where,
                                        uint64_t* out_kmers /*[h|d] u64[2n]*/, uint32_t* out_pos /*[h|d]*/, uint64_t* n_out, int device, void* hip_stream);
kh_status kh_kmers128_from_fastq_pos(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, int canonical, kh_mem where,
                                     uint64_t* out_kmers /*[h|d] u64[2n]*/, uint32_t* out_pos /*[h|d]*/, uint64_t* n_out, int device, void* hip_stream);

/* ---- (w,k)-minimizer sampling: the k-mers a seed index keeps instead of every window (the reference tree has no sampler -- its parser
 *      and multimap are kmerind's and absent --: the definition below is this library's).
 *      Inputs: a text, k (1..32), w (1..256), `canonical`, an ordering hash `order_hash` and `order_seed`.
 *      - Valid windows, k-mers and positions are exactly those of kh_kmers_from_sequence_pos (packing, canonical form, byte offsets).
 *      - Order key of the valid window at offset p: h(p) = the hash `order_hash` with seed `order_seed` of the EMITTED k-mer (of the
 *        canonical form when `canonical` is set): the value kh_hash_batch gives for it.
 *      - Full window: a start offset s is a full window iff all w offsets s .. s + w - 1 are valid window starts, i.e. the w + k - 1
 *        bytes from s are all bases.  A window never spans a non-base byte, a newline or two reads.
 *      - Selection: the pick of a full window s is the offset p in [s, s + w) with the smallest (h(p), p): ties on the hash go to the
 *        LEFTMOST offset.
 *      - Output: an offset is emitted ONCE if at least one full window picks it; the pairs (k-mer, offset) come out in ascending
 *        offset order.  A run of fewer than w + k - 1 bases yields nothing.  w = 1: the output of kh_kmers_from_sequence_pos, byte for byte.
 *      Equivalently, p is emitted iff it is valid and L + R + 1 >= w, where L counts the consecutive valid offsets directly left of p
 *      with h > h(p) and R those directly right of p with h >= h(p), both capped at w - 1.
 *      Two texts that share w + k - 1 bases share a sampled k-mer at the same place of that stretch; about 2 / (w + 1) of the windows
 *      of a random text are kept.  REPEATS: in a stretch of equal k-mers (poly-A) every hash ties, the leftmost rule picks every
 *      full-window start in it, and nothing is thinned there -- mask such k-mers in the index afterwards (kh_index_erase_counts).
 *      The ordering hash is an argument of its own: the index's table takes its home bucket from hash & mask, and selecting the small
 *      values of the SAME seeded hash would fill the low buckets of a small table first; choose a different hash or seed.
 *      out_kmers == NULL: count only -- *n_out is set, nothing is written, only the count pass and the scan run.  Otherwise cap_out is
 *      the room offered in out_kmers and out_pos (both required); more picks than cap_out: KH_ERR_INVALID with *n_out set and the
 *      outputs untouched (the total is known before anything is written, as for kh_index_find).  KH_ERR_INVALID before anything is
 *      allocated or read: k outside 1..32, w outside 1..256, n >= 2^32, an unknown hash, NULL text with n > 0, NULL n_out.  n == 0 or
 *      a text shorter than w + k - 1: KH_OK and *n_out = 0.  kh_minimizers_from_fastq: the sequence lines of raw FASTQ text, as
 *      kh_kmers_from_fastq_pos reads them (offsets into the raw text).  Two passes over the text, 1 B per base read each, 12 B per
 *      EMITTED pair written; no hash array in device memory. */
kh_status kh_minimizers_from_sequence(const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t w /*1..256*/, int canonical,
                                      kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                      uint64_t* out_kmers /*[h|d] or NULL*/, uint32_t* out_pos /*[h|d] or NULL*/, uint64_t cap_out,
                                      uint64_t* n_out, int device, void* hip_stream);
kh_status kh_minimizers_from_fastq(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t w /*1..256*/, int canonical,
                                   kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                   uint64_t* out_kmers /*[h|d] or NULL*/, uint32_t* out_pos /*[h|d] or NULL*/, uint64_t cap_out,
                                   uint64_t* n_out, int device, void* hip_stream);
/* a position index over the minimizers of a text (fastq != 0: raw FASTQ text): the pairs of kh_minimizers_from_sequence / _fastq, with
 *      pos_base added to every offset on the device, followed by kh_index_build / kh_index_append -- the export is byte-identical to
 *      kh_index_build over those pairs.  The pair buffers are sized from the count pass, NOT from n: peak staging is 12 B per emitted
 *      pair (next to the text copy of a host text and the FASTQ mask).  Failure states and refusals are those of
 *      kh_index_append_from_sequence, plus w out of range and an unknown order hash; 16-byte k-mers (kh_windex) are not supported. */
kh_status kh_index_build_from_minimizers(kh_index* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t w /*1..256*/, int canonical,
                                         kh_hash order_hash, uint64_t order_seed, kh_mem where, int fastq);
kh_status kh_index_append_from_minimizers(kh_index* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t w /*1..256*/, int canonical,
                                          kh_hash order_hash, uint64_t order_seed, kh_mem where, int fastq, uint32_t pos_base);

/* ---- closed-syncmer sampling (Edgar 2021): a sampler whose choice is a function of the k-mer ALONE, for both key widths (k = 1..32 in
 *      8-byte k-mers, k = 1..64 in 16-byte k-mers {w0, w1}).  The reference tree has no sampler: the definition below is this library's.
 *      Inputs: a text, k, s with 1 <= s <= min(k, 32), `canonical`, an ordering hash `order_hash` and `order_seed`.
 *      - Valid windows, packing, canonical form, offsets and FASTQ masking are exactly those of kh_kmers_from_sequence_pos
 *        (kh_kmers128_from_sequence_pos for the 128 forms).
 *      - Order key of offset i: h(i) = the hash `order_hash` with seed `order_seed` of the s-mer that starts at i, packed as a k-mer of
 *        length s is (64 bits: s <= 32 for either key width), of its canonical form when `canonical` is set: the value kh_hash_batch
 *        gives for it.
 *      - Selection: let m be the smallest order key among the k - s + 1 offsets p .. p + k - s.  The k-mer of the valid window p is KEPT
 *        iff h(p) == m or h(p + k - s) == m: its smallest s-mer is its first or its last.  A tie with an inner s-mer still keeps it.
 *        With canonical s-mers the reverse complement of a k-mer sees the same keys in the opposite order, and the inclusive tie rule
 *        makes the choice exactly strand-symmetric: a text and its reverse complement keep the same canonical k-mers at mirrored places.
 *      - Output: the kept windows in ascending offset, each once; (k-mer, position) is what the all-window front end emits for it.
 *      s == k keeps every window: the output of kh_kmers_from_sequence_pos (kh_kmers128_...), byte for byte.  About 2 / (k - s + 1) of
 *      the k-mers of a random text are kept (not for very small s, where few distinct keys tie constantly).  Selection does not depend
 *      on the neighbours: a run of k bases yields its k-mer if that k-mer is a syncmer, and kh_syncmer_mask answers for any k-mer, with
 *      no text, whether a sampled index CAN hold it.  REPEATS: in a homopolymer every key ties and every window is kept, as with
 *      minimizers -- mask such k-mers afterwards (kh_index_erase_counts).  Choose an ordering hash or seed other than the table's.
 *      out_kmers == NULL: count only -- *n_out is set, nothing is written.  Otherwise cap_out is the room offered in out_kmers
 *      (u64[cap_out], u64[2 cap_out] for the 128 forms) and out_pos (both required); more kept windows than cap_out: KH_ERR_INVALID with
 *      *n_out set and the outputs untouched.  KH_ERR_INVALID before anything is allocated or read: s == 0, s > k, s > 32, k outside
 *      1..32 (1..64), n >= 2^32, an unknown hash, NULL text with n > 0, NULL n_out.  n == 0 or a text shorter than k: KH_OK and
 *      *n_out = 0.  Two passes over the text, 1 B per base read each, 12 B (20 B) per KEPT pair written; no hash array in device memory. */
kh_status kh_syncmers_from_sequence(const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t s /*1..k*/, int canonical,
                                    kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                    uint64_t* out_kmers /*[h|d] or NULL*/, uint32_t* out_pos /*[h|d] or NULL*/, uint64_t cap_out,
                                    uint64_t* n_out, int device, void* hip_stream);
kh_status kh_syncmers_from_fastq(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t s /*1..k*/, int canonical,
                                 kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                 uint64_t* out_kmers /*[h|d] or NULL*/, uint32_t* out_pos /*[h|d] or NULL*/, uint64_t cap_out,
                                 uint64_t* n_out, int device, void* hip_stream);
kh_status kh_syncmers128_from_sequence(const void* seq /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, uint32_t s /*1..min(k,32)*/, int canonical,
                                       kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                       uint64_t* out_kmers /*[h|d] u64[2 cap_out] or NULL*/, uint32_t* out_pos /*[h|d] or NULL*/, uint64_t cap_out,
                                       uint64_t* n_out, int device, void* hip_stream);
kh_status kh_syncmers128_from_fastq(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, uint32_t s /*1..min(k,32)*/, int canonical,
                                    kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                    uint64_t* out_kmers /*[h|d] u64[2 cap_out] or NULL*/, uint32_t* out_pos /*[h|d] or NULL*/, uint64_t cap_out,
                                    uint64_t* n_out, int device, void* hip_stream);
/* the selection alone, on a batch of packed k-mers (as the front ends and the tables hold them; bits above 2k are ignored):
 *      out_mask[i] = 1 iff key i is a closed syncmer under (k, s, canonical, order_hash, order_seed), else 0; out_mask lives where the keys
 *      live.  With `canonical` a k-mer and its reverse complement give the same answer.  Refusals as above (no n_out); n == 0: KH_OK;
 *      NULL out_mask with n > 0: KH_ERR_INVALID.  Synchronous. */
kh_status kh_syncmer_mask(const void* keys /*[h|d] u64[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t s /*1..k*/, int canonical,
                          kh_hash order_hash, uint64_t order_seed, kh_mem where, uint8_t* out_mask /*[h|d] u8[n]*/, int device, void* hip_stream);
kh_status kh_wide_syncmer_mask(const void* keys /*[h|d] u64[2n]*/, uint64_t n, uint32_t k /*1..64*/, uint32_t s /*1..min(k,32)*/, int canonical,
                               kh_hash order_hash, uint64_t order_seed, kh_mem where, uint8_t* out_mask /*[h|d] u8[n]*/, int device, void* hip_stream);
/* a position index over the closed syncmers of a text (fastq != 0: raw FASTQ text), either key width: the route of
 *      kh_index_build_from_minimizers -- count pass, pair buffers of exactly that size (12 B or 20 B per kept pair), emit pass with
 *      pos_base added on the device, then kh_index_build / kh_index_append of the pairs, to which the export is byte-identical.
 *      Failure states and refusals are those of kh_index_append_from_sequence, plus s out of range and an unknown order hash. */
kh_status kh_index_build_from_syncmers(kh_index* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t s /*1..k*/, int canonical,
                                       kh_hash order_hash, uint64_t order_seed, kh_mem where, int fastq);
kh_status kh_index_append_from_syncmers(kh_index* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..32*/, uint32_t s /*1..k*/, int canonical,
                                        kh_hash order_hash, uint64_t order_seed, kh_mem where, int fastq, uint32_t pos_base);
kh_status kh_wide_index_build_from_syncmers(kh_windex* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, uint32_t s /*1..min(k,32)*/,
                                            int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where, int fastq);
kh_status kh_wide_index_append_from_syncmers(kh_windex* x, const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, uint32_t s /*1..min(k,32)*/,
                                             int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where, int fastq, uint32_t pos_base);

/* a CSR that arrives in a permuted order, back into query order (the last step of a sharded find: the answers return grouped by owner
 *      rank, in the permuted order of kh_shard_permute with vals = 0..n-1).
 * counts_perm[j] and the segments of pos_perm (concatenated in order j = 0..n-1) belong to the query whose index in the caller's
 * batch is origin[j]; origin is a permutation of 0..n-1 (precondition, not checked).  Writes the CSR in QUERY order:
 * out_counts[i] (may be NULL), out_offsets[0..n] = exclusive scan (may be NULL), out_pos = the segments in query order (may be
 * NULL: counts / offsets / *n_out only).  *n_out = total.  total > cap_out with out_pos != NULL: KH_ERR_INVALID, *n_out and the
 * offsets set, out_pos untouched (the convention of kh_index_find).  Device buffers only; n == 0 and total == 0 are KH_OK.
 * n or total >= 2^32: KH_ERR_INVALID before anything is touched.  Synchronous: the stream has drained when the call returns. */
kh_status kh_csr_unpermute(const uint32_t* counts_perm, const uint32_t* pos_perm, const uint32_t* origin, uint64_t n,
                           uint32_t* out_counts, uint64_t* out_offsets, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out,
                           int device, void* hip_stream);

/* ---- strand of a window position, stranded indexes, anchors.  Every canonical front end emits min(k-mer, reverse complement) and the
 *      window's offset; which of the two it emitted is a function of the text window alone and is recovered here, by one pass over
 *      (text, positions) that serves every front end, both samplers and both key widths.
 *      Definition.  For a text of n bytes, k in 1..64 and a position p, the window at p is VALID iff p + k <= n and its k bytes are bases
 *      (ACGT in either case, as every front end reads them).  Its strand bit rc(p) is 1 iff the reverse complement of the window is
 *      STRICTLY smaller than the window (A=0 C=1 G=2 T=3, first base most significant): exactly the case in which `canonical` makes the
 *      front ends emit the reverse complement.  A palindrome has rc = 0.  The STAMPED position is v = ((pos_base + p) << 1) | rc(p);
 *      stamped values sort like positions; position = v >> 1, strand = v & 1.  An invalid window gives KH_POS_INVALID.  The stamped
 *      coordinate space is 2^31 (64-bit positions are not supported).  The definition is on bytes and knows nothing of FASTQ structure:
 *      the positions the FASTQ front ends emit are raw-text offsets of windows that lie in one sequence line and qualify as they are.
 *      kh_stamp_strand: text, pos and out live in the memory `where` names (device pointers valid on `device`); positions may come in
 *      any order and may repeat; out may alias pos; no byte outside [text, text + n) is ever read, whatever pos holds.  *n_invalid
 *      receives the number of KH_POS_INVALID written.  Device memory with n_invalid == NULL: the call only queues its work on
 *      hip_stream (inputs must stay valid until it has run); a non-NULL n_invalid, or host memory, synchronises the stream.
 *      KH_ERR_INVALID before anything is allocated or read: k outside 1..64, n >= 2^31, pos_base + n > 2^31, a null pos or out (or a
 *      null text with n > 0) while m > 0.  m == 0: KH_OK. */
#define KH_POS_INVALID 0xFFFFFFFFu
kh_status kh_stamp_strand(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t k /*1..64*/, const uint32_t* pos /*[h|d] u32[m]*/, uint64_t m,
                          uint32_t pos_base, kh_mem where, uint32_t* out /*[h|d] u32[m], may alias pos*/, uint64_t* n_invalid /* may be NULL */,
                          int device, void* hip_stream);
/*      A STRANDED index stores stamped positions in every text form: kh_[wide_]index_build_from_sequence / _from_fastq,
 *      _append_from_sequence / _from_fastq, and the _from_minimizers and _from_syncmers forms take the front end's pairs with pos_base 0
 *      and stamp them over the device text they already hold (the stamp takes the place of the pass that adds pos_base).  Allowed only
 *      on an empty index (size 0, total 0): otherwise KH_ERR_INVALID and the index is unchanged.  The flag survives kh_index_clear and a
 *      failed build.  On a stranded index the text forms refuse, before the index is touched: canonical == 0, n >= 2^31,
 *      pos_base + n > 2^31.  kh_index_build / kh_index_append over caller-supplied pairs are unchanged (the caller stamps: kh_stamp_strand),
 *      and so are find, count, export, erase* -- they never interpret a position; find and export return the stamped values, which
 *      ascend per key as positions do.  An index that is not stranded launches exactly the kernels it launched before. */
kh_status kh_index_set_stranded(kh_index* x, int on);
kh_status kh_wide_index_set_stranded(kh_windex* x, int on);
/*      kh_anchors_from_csr: the CSR of a find over a stranded index (stamped query positions qpos[n], offsets[n + 1] with offsets[0] = 0
 *      and offsets[n] = total, stamped hits pos[total]) into the flat anchor list a chainer consumes.  For output j in row i
 *      (offsets[i] <= j < offsets[i + 1]): out_qpos[j] = qpos[i] >> 1, out_rpos[j] = pos[j] >> 1, out_rev[j] = (qpos[i] ^ pos[j]) & 1 --
 *      0: the k bases at out_rpos in the reference equal those at out_qpos in the query, 1: they are its reverse complement.  Empty
 *      rows give nothing.  Handle-free, like kh_csr_unpermute; all arrays live in the memory `where` names; device memory: the call only
 *      queues its work on hip_stream.  total >= 2^32: KH_ERR_INVALID; n == 0 or total == 0: KH_OK, nothing written; a null array
 *      otherwise: KH_ERR_INVALID. */
kh_status kh_anchors_from_csr(const uint32_t* qpos /*[h|d] u32[n]*/, const uint64_t* offsets /*[h|d] u64[n+1]*/, uint64_t n,
                              const uint32_t* pos /*[h|d] u32[total]*/, uint64_t total, kh_mem where, uint32_t* out_qpos /*[h|d] u32[total]*/,
                              uint32_t* out_rpos /*[h|d] u32[total]*/, uint8_t* out_rev /*[h|d] u8[total]*/, int device, void* hip_stream);

/* ---- collinear chains from anchors.  kh_chain_anchors takes a flat anchor list (qpos, rpos, rev: what kh_anchors_from_csr writes) and a
 *      CSR of SEGMENTS -- segment s is the anchors [seg_offsets[s], seg_offsets[s + 1]), one read; NULL: one segment [0, m) -- and returns
 *      the chaining DP per anchor, a partition of the anchors into disjoint chains and a compact table of the chains that pass a filter.
 *      Chains never cross a segment boundary.  No order of the anchors inside a segment is assumed (query order makes good chains).
 *      DP, inside a segment [a, b), i ascending.  Only bit 0 of rev is read.  An anchor with qpos >= 2^31 or rpos >= 2^31 (KH_POS_INVALID)
 *      has f = k, pred = -1 and is nobody's candidate.  Candidates of i are the j with max(a, i - lookback) <= j < i, rev[j] == rev[i],
 *      dq = q_i - q_j in 1..max_gap, dr in 1..max_gap (dr = r_i - r_j for rev 0, r_j - r_i for rev 1) and dd = |dq - dr| <= band.
 *      cand = f(j) + min(dq, dr, k) - cost(dd), cost(0) = 0, cost(dd) = ((k * dd) >> 7) + (floor(log2 dd) >> 1).  f(i) = max(k, max cand);
 *      pred(i) = the candidate of greatest cand if that cand > k (ties: the largest j), else -1.
 *      Chains.  g(i) = max(f(i), g(c) over the c with pred(c) == i); best_child(j) = the child of greatest g (ties: the smallest index).
 *      Anchor i STARTS a chain iff pred(i) == -1 or best_child(pred(i)) != i, else it belongs to the chain of pred(i): every anchor lies in
 *      exactly one chain and a chain is a path of pred links.  For a chain with start s and last anchor l: count = its anchors, score =
 *      f(l) - (pred(s) == -1 ? 0 : f(pred(s))).  It is KEPT iff score >= min_score and count >= min_count; kept chains are numbered from 0
 *      in ascending order of their start anchor.
 *      Outputs: out_score[i] = f(i), out_pred[i] = pred(i), out_chain[i] = the number of i's chain or -1 when it is not kept; row c of the
 *      table: c_first, c_last (start and last anchor), c_count, c_score.  c_* all NULL: per-anchor outputs and the count only.
 *      *n_chains = number of kept chains; the call waits for the stream to learn it (device memory: every kernel is queued on hip_stream
 *      and that wait is the only one).  More kept chains than cap_chains (with a table): KH_ERR_INVALID, *n_chains set, per-anchor outputs
 *      written, c_* untouched -- the cap_out convention of kh_index_find.  All arrays live in the memory `where` names.
 *      KH_ERR_INVALID before anything is allocated, read or written: k or lookback outside 1..64, max_gap outside 1..2^31-1, band >= 2^31,
 *      m > 2^24 (scores stay within 2^30; batch over reads), some but not all of c_* NULL, and while m > 0 a null input or per-anchor
 *      output, n_seg > m + 2^24 or n_seg == 0 with seg_offsets given.  m == 0: KH_OK, *n_chains = 0.  seg_offsets that do not ascend from 0
 *      to m are seen on the device only: every segment is clamped to [0, m) so nothing outside the arrays is touched, and the call
 *      returns KH_ERR_INVALID with *n_chains = 0 and unspecified output contents. */
kh_status kh_chain_anchors(const uint32_t* qpos /*[h|d] u32[m]*/, const uint32_t* rpos /*[h|d] u32[m]*/, const uint8_t* rev /*[h|d] u8[m]*/, uint64_t m,
                           const uint64_t* seg_offsets /*[h|d] u64[n_seg+1] or NULL*/, uint64_t n_seg, uint32_t k /*1..64*/, uint32_t lookback /*1..64*/,
                           uint32_t max_gap /*1..2^31-1*/, uint32_t band /*0..2^31-1*/, int32_t min_score, uint32_t min_count, kh_mem where,
                           int32_t* out_score /*[m]*/, int32_t* out_pred /*[m], -1 = none*/, int32_t* out_chain /*[m], kept-chain number or -1*/,
                           uint32_t* c_first, uint32_t* c_last, uint32_t* c_count, int32_t* c_score /* each [cap_chains], or all NULL */,
                           uint64_t cap_chains, uint64_t* n_chains, int device, void* hip_stream);

/* ---- edit distance per chain.  kh_chain_edits verifies the chains of kh_chain_anchors against the two texts: the unit-cost (Levenshtein)
 *      distance of every link of every kept chain, and per chain their sum.  Inputs: the query text qtext[nq]; the reference text
 *      rtext[nr], which covers the reference coordinates [ref_base, ref_base + nr) (an index keeps no text: the caller supplies it); the
 *      anchors qpos, rpos, rev [m]; pred and chain [m] as kh_chain_anchors wrote them; n_chains, k, max_edits.
 *      Bases.  A/a = 0, C/c = 1, G/g = 2, T/t = 3, any other byte = 4.  Two bases MATCH iff both codes are < 4 and equal; on the reverse
 *      strand iff both are < 4 and sum to 3.  An N matches nothing, another N included.
 *      Links.  Anchor i HAS A LINK iff 0 <= chain[i] < n_chains, 0 <= pred[i] < i and chain[pred[i]] == chain[i]: it continues its
 *      predecessor's kept chain.  With j = pred[i], dq = q_i - q_j and the strand taken from bit 0 of rev[i]:
 *        forward: dr = r_i - r_j, A = qtext[q_j, q_i), B = rtext[r_j - ref_base, r_i - ref_base);
 *        reverse: dr = r_j - r_i, A as above, B = the reverse complement of rtext[r_i + k - ref_base, r_j + k - ref_base)
 *      -- the stretch of reference A faces, given that the k bases at r_j are the reverse complement of the k at q_j.  Both strings start
 *      at the seed of anchor j; the last anchor of a chain adds its k matching bases and nothing else.
 *      out_link[i] = KH_EDITS_NOLINK: i has no link.  KH_EDITS_OVER: a position is >= 2^31; or dq < 1, dr < 1, q_i + k > nq, or a bound
 *      of B's stretch of rtext (with its + k on the reverse strand) lies outside [0, nr]; or |dq - dr| > max_edits; or lev(A, B) >
 *      max_edits.  Otherwise lev(A, B), the Levenshtein distance under the match rule above (substitution, insertion, deletion: 1 each).
 *      c_edits[c] = the sum of out_link over the links of chain c that are >= 0, c_over[c] = the number of its KH_EDITS_OVER links; the
 *      call zeroes both arrays [n_chains] first.  No byte outside the two texts is ever read, whatever the arrays hold, and no element
 *      outside the arrays is written.
 *      Route: one lane per anchor settles NOLINK, the range checks and the links with dq == dr whose strings match exactly; the others
 *      go through a furthest-reaching-point (Landau-Vishkin) pass, one wavefront per link with one diagonal per lane, which is why
 *      max_edits <= 31 (kh_kernels_edits.h fixes the orientation).
 *      All arrays live in the memory `where` names.  Device memory: the call only queues work on hip_stream and never waits -- there is
 *      no count to return, and bad input becomes NOLINK / OVER, not an error word; its scratch block returns to the pool from a host function
 *      queued behind the kernels.  The call is not capturable into a graph: on a capturing stream it waits like a host call (and so
 *      ends the capture with an error).  Host memory: staged, and the call synchronises.
 *      KH_ERR_INVALID before anything is allocated, read or written: k outside 1..64, max_edits > 31, m > 2^24, nq >= 2^31,
 *      ref_base + nr > 2^31, `where` outside the enum, n_chains > 0 with a null c_edits or c_over, and while m > 0 a null array or a null
 *      text of positive length.  m == 0: KH_OK, c_edits and c_over zeroed if n_chains > 0. */
#define KH_EDITS_NOLINK (-1)
#define KH_EDITS_OVER (-2)
kh_status kh_chain_edits(const void* qtext /*[h|d] u8[nq]*/, uint64_t nq, const void* rtext /*[h|d] u8[nr]*/, uint64_t nr, uint32_t ref_base,
                         const uint32_t* qpos /*[h|d] u32[m]*/, const uint32_t* rpos /*[h|d] u32[m]*/, const uint8_t* rev /*[h|d] u8[m]*/,
                         const int32_t* pred /*[h|d] i32[m]*/, const int32_t* chain /*[h|d] i32[m]*/, uint64_t m, uint64_t n_chains,
                         uint32_t k /*1..64*/, uint32_t max_edits /*0..31*/, kh_mem where, int32_t* out_link /*[m]*/,
                         uint32_t* c_edits /*[n_chains]*/, uint32_t* c_over /*[n_chains]*/, int device, void* hip_stream);

/* ---- alignment operations per chain.  kh_chain_cigars says WHICH edits kh_chain_edits counted: for every link a run-length alignment
 *      of A against B, found by the traceback of the same furthest-reaching-point pass.  Inputs: those of kh_chain_edits (texts, anchors,
 *      pred, chain, n_chains, k; links, strings A and B, orientation and the match rule are defined there) and link[m], the out_link
 *      array that call wrote over the same inputs.
 *      Output: a CSR in anchor order.  Row i = out_ops[out_offsets[i] .. out_offsets[i + 1]) describes how A = qtext[q_j, q_i) becomes
 *      B, the reference stretch A faces (reverse-complemented on the reverse strand), read from the seed of anchor j = pred[i] forwards.
 *      Each run is one uint32 in BAM encoding, (len << 4) | op, with op I = 1 (a base of A that B lacks), D = 2 (a base of B that A
 *      lacks), '=' = 7 (matching bases) and X = 8 (a substitution).  Adjacent runs of a row never share an op; a row has at most
 *      2 link[i] + 1 runs.
 *      Which rows are non-empty.  Row i is empty unless anchor i has a link that passes the range checks of kh_chain_edits with
 *      max_edits = 31 -- 0 <= chain[i] < n_chains, 0 <= pred[i] < i, chain[pred[i]] == chain[i]; all four positions < 2^31; dq >= 1,
 *      dr >= 1, q_i + k <= nq, B's stretch of rtext (with its + k on the reverse strand) inside [0, nr]; |dq - dr| <= 31 -- and unless
 *      0 <= link[i] <= 31, dq < 2^28 and dr < 2^28.  Then:
 *        link[i] == 0 and dq == dr: the single run "dq =".  The texts are not read.
 *        link[i] == 0 and dq != dr: an empty row.
 *        link[i] > 0: the canonical alignment below, looked for among the distances 0..link[i].  If the target is reached at a smaller
 *        e than link[i], that alignment is the row; if it is not reached by link[i], the row is empty.
 *      Garbage in link, pred or chain therefore yields empty or wrong rows; it never causes a read outside the texts or a write outside
 *      the arrays.
 *      Canonical alignment.  Fixed on the furthest-reaching points, so that it depends on no scheduling and tests/cigar_model.py equals
 *      it bit for bit.  n = |A|, mB = |B|; diagonal d = (offset in B) - (offset in A), -31..31; hi(d) = min(n, mB - d); ext(v, d) = the
 *      offset in A after the run of matching bases from v on d, at most hi(d) (an N matches nothing).  F_0[0] = ext(0, 0), every other
 *      diagonal is unreached.  For e >= 1 the candidates of d are  X: F_{e-1}[d] + 1,  I: F_{e-1}[d+1] + 1,  D: F_{e-1}[d-1];  a
 *      candidate is valid iff its source is reached and its value v satisfies v <= hi(d) and v + d >= 0 -- an invalid one is dropped,
 *      not clamped: a clamped value is no real edit and cannot be traced back.  pre_e[d] = the greatest valid candidate, the MOVE of
 *      (e, d) the first of X, I, D that attains it, F_e[d] = ext(pre_e[d], d).  The alignment is complete at the first e with
 *      F_e[mB - n] == n; the traceback follows the moves from (e, mB - n) to (0, 0).  Read forwards the row is F_0[0] '=', then per
 *      level t one base of its move and F_t[d_t] - pre_t[d_t] of '='; zero lengths are dropped and equal neighbours merged.
 *      c_ins[c] and c_del[c] = the I and D bases summed over the non-empty rows of chain c; the call zeroes both arrays [n_chains]
 *      first.  With c_edits they give a chain's mismatches (edits - I - D), its matched bases (q_end - q_start - X - I) and its
 *      alignment block length without a look at the ops.
 *      All arrays live in the memory `where` names.  out_ops == NULL: count only -- out_offsets, *n_ops and the chain arrays are
 *      written.  More runs than cap_ops: KH_ERR_INVALID with *n_ops set, out_offsets written and out_ops untouched.  Device memory:
 *      everything is queued on hip_stream and the one host wait is the one that learns *n_ops.  Host memory: staged, the call synchronises.
 *      KH_ERR_INVALID before anything is allocated, read or written: k outside 1..64, m > 2^24, nq >= 2^31, ref_base + nr > 2^31, `where`
 *      outside the enum, n_chains > 0 with a null c_ins or c_del, a null out_offsets or n_ops, and while m > 0 a null array (link
 *      included) or a null text of positive length.  m == 0: KH_OK, *n_ops = 0, out_offsets[0] = 0, c_ins and c_del zeroed. */
kh_status kh_chain_cigars(const void* qtext /*[h|d] u8[nq]*/, uint64_t nq, const void* rtext /*[h|d] u8[nr]*/, uint64_t nr, uint32_t ref_base,
                          const uint32_t* qpos /*[h|d] u32[m]*/, const uint32_t* rpos /*[h|d] u32[m]*/, const uint8_t* rev /*[h|d] u8[m]*/,
                          const int32_t* pred /*[h|d] i32[m]*/, const int32_t* chain /*[h|d] i32[m]*/, uint64_t m, uint64_t n_chains,
                          uint32_t k /*1..64*/, const int32_t* link /*[h|d] i32[m], out_link of kh_chain_edits*/, kh_mem where,
                          uint64_t* out_offsets /*[m+1]*/, uint32_t* out_ops /*[cap_ops] or NULL*/, uint64_t cap_ops, uint64_t* n_ops,
                          uint32_t* c_ins /*[n_chains]*/, uint32_t* c_del /*[n_chains]*/, int device, void* hip_stream);

/* ---- the ends of every chain.  kh_chain_edits and kh_chain_cigars stop at the seeds: a chain's alignment covers the read from its first
 *      seed's first base to its last seed's last base.  kh_chain_ends looks at the rest of the read: from either outermost seed it
 *      extends the alignment outwards until the read ends or until stopping scores better (a soft clip), and says how far it came, at
 *      what cost, and by which operations.  Inputs: the two texts with ref_base and the anchors qpos, rpos, rev [m] as for
 *      kh_chain_edits (bases and the match rule are defined there: an N matches nothing); c_first, c_last [n_chains], the anchor
 *      indices of each kept chain's first and last anchor as kh_chain_anchors wrote them; q_lo, q_hi [n_chains], the byte interval
 *      [q_lo, q_hi) of the chain's read in qtext; k, max_edits (0..31) and clip_cost (1..255; 4 is a usual value).
 *      Rows.  Chain c has two ends: row 2c is its HEAD, the part of the read before its first seed, row 2c + 1 its TAIL, the part behind
 *      its last seed.  With f = c_first[c], l = c_last[c], the strand taken from bit 0 of rev[f] for the head and of rev[l] for the
 *      tail, both strings run AWAY from the seed:
 *        tail, A = qtext[q_l + k, q_hi) read upwards;  B forward: rtext read upwards from r_l + k - ref_base;  B reverse: the complement
 *              of rtext read downwards from r_l - ref_base - 1;
 *        head, A = qtext[q_lo, q_f) read DOWNWARDS from q_f - 1;  B forward: rtext read downwards from r_f - ref_base - 1 (no
 *              complement);  B reverse: the complement of rtext read upwards from r_f + k - ref_base.
 *      n = |A|; |B| = min(n + max_edits, the bases rtext has left in that direction).
 *      Which rows are looked at.  With x = f for the head and x = l for the tail, a row is EMPTY -- no runs, all four numbers 0 --
 *      unless x < m; q_x < 2^31 and r_x < 2^31; the seed lies inside the read and the read inside the text, q_lo <= q_x and
 *      q_x + k <= q_hi <= nq; the seed lies inside rtext, ref_base <= r_x and r_x + k - ref_base <= nr; and 1 <= n < 2^28.  (n == 0: the
 *      seed touches the read's end; nothing is left to align and e_clip is 0.)  Garbage in the arrays therefore yields empty or wrong
 *      rows; no byte outside the two texts is ever read and no element outside the arrays is written.
 *      Extension.  The furthest-reaching points F_e[d] are those of the canonical alignment of kh_chain_cigars, word for word: diagonal
 *      d = (offset in B) - (offset in A), -31..31; hi(d) = min(n, |B| - d); F_0[0] = ext(0, 0); candidates X, I, D, an invalid one
 *      dropped, not clamped; the move of (e, d) the first of X, I, D that attains the greatest valid candidate.  What differs is the
 *      target: A must be used up, B may end anywhere, and the alignment may stop early.  Levels e = 0..E are computed, E = the first
 *      level at which some diagonal holds n, or max_edits if none does.  Every reached point scores S(e, d) = F_e[d] - clip_cost * e:
 *      one for each base of the read it aligns, clip_cost off for each edit.  The end's alignment stops at the point of greatest S; ties
 *      go to the smaller e, then to the smaller |d|, then to d < 0.  (0, 0) is always reached, so an end never scores below its
 *      exact-match extension.  Stopping at E loses nothing: F never exceeds n, so a later level scores below n - clip_cost * E.
 *      Outputs per row: e_q = F at that point, the bases of the read that are aligned; e_r = F + d, the bases of the reference they
 *      face; e_edits = e; e_clip = n - F, the bases of the read left over (a soft clip); and a CSR row of runs in the BAM encoding of
 *      kh_chain_cigars (I, D, =, X -- no S: e_clip says it), found by the traceback from that point to (0, 0).  A tail's row is stored
 *      as it is found, from the seed outwards.  A HEAD's row is stored in READ order, the reverse of the order in which it is found --
 *      so head row, the chain's link rows, k '=' for the last seed and tail row concatenate to the CIGAR of the whole read.  Adjacent
 *      runs never share an op; a row has at most 2 e_edits + 1 <= 63 runs.
 *      All arrays live in the memory `where` names.  out_ops == NULL: count only -- the four numbers, out_offsets [2 n_chains + 1] and
 *      *n_ops are written.  More runs than cap_ops: KH_ERR_INVALID with *n_ops set, the numbers and out_offsets written and out_ops
 *      untouched.  Device memory: everything is queued on hip_stream and the one host wait is the one that learns *n_ops.  Host memory:
 *      staged, the call synchronises.
 *      KH_ERR_INVALID before anything is allocated, read or written: k outside 1..64, max_edits > 31, clip_cost outside 1..255,
 *      m > 2^24, n_chains > 2^23, nq >= 2^31, ref_base + nr > 2^31, `where` outside the enum, a null out_offsets or n_ops, while
 *      n_chains > 0 a null chain array or output, and while both n_chains > 0 and m > 0 a null anchor array or a null text of positive
 *      length.  n_chains == 0: KH_OK, *n_ops = 0, out_offsets[0] = 0. */
kh_status kh_chain_ends(const void* qtext /*[h|d] u8[nq]*/, uint64_t nq, const void* rtext /*[h|d] u8[nr]*/, uint64_t nr, uint32_t ref_base,
                        const uint32_t* qpos /*[h|d] u32[m]*/, const uint32_t* rpos /*[h|d] u32[m]*/, const uint8_t* rev /*[h|d] u8[m]*/, uint64_t m,
                        const uint32_t* c_first /*[h|d] u32[n_chains]*/, const uint32_t* c_last /*[h|d] u32[n_chains]*/,
                        const uint32_t* q_lo /*[h|d] u32[n_chains]*/, const uint32_t* q_hi /*[h|d] u32[n_chains]*/, uint64_t n_chains,
                        uint32_t k /*1..64*/, uint32_t max_edits /*0..31*/, uint32_t clip_cost /*1..255*/, kh_mem where,
                        uint32_t* e_q, uint32_t* e_r, uint32_t* e_edits, uint32_t* e_clip /* each [2 n_chains] */,
                        uint64_t* out_offsets /*[2 n_chains + 1]*/, uint32_t* out_ops /*[cap_ops] or NULL*/, uint64_t cap_ops, uint64_t* n_ops,
                        int device, void* hip_stream);

/* ---- primary chains and a mapping quality.  The calls above leave a read that touches a repeat as several chains; kh_chain_select says
 *      which of them is the answer, which are alternatives worth keeping, and how sure the answer is.  Integers only, no floating point
 *      anywhere: the kernels equal the model of tests/select_model.py bit for bit.
 *      Inputs.  n_chains chains; chain c has a query interval [q_start[c], q_end[c]) (u32), a score s_c (i32, any value) and an anchor
 *      count cnt_c (u32).  A CSR of GROUPS -- group g is the chains [offsets[g], offsets[g + 1]), one read; offsets == NULL: one group
 *      [0, n_chains).  (kh_chain_anchors numbers chains by their start anchor, so the chains of a read already form a contiguous run.)
 *      Parameters mask_pct 0..100 (usual value 50), pri_pct 0..100 (80), best_n (5).
 *      Rank.  Inside a group, chains are ordered by score descending, ties to the smaller chain number; rank_c is the 0-based position
 *      of c in that order.
 *      Overlap, all arithmetic in signed 64-bit.  len_c = max(0, qe_c - qs_c); ov(c, p) = max(0, min(qe_c, qe_p) - max(qs_c, qs_p));
 *      p COVERS c iff 100 * ov(c, p) >= mask_pct * min(len_c, len_p).  So a chain of length 0 is covered by anything, and mask_pct = 0
 *      means one primary per read.
 *      Primaries.  Take the chains of a group in rank order.  Chain c is SECONDARY if an earlier chain that is itself primary covers it;
 *      its parent is then the covering primary of smallest rank.  Otherwise c is PRIMARY and parent_c = c.  A secondary never covers
 *      anything.
 *      Per primary p: nsub_p = the number of its secondaries; sub_p = max(0, the greatest score among them), 0 when it has none;
 *      mapq_p = 0 if s_p <= 0, otherwise
 *        mapq_p = min(60, floor(60 * (s_p - sub_p) * min(cnt_p, 10) * min(s_p, 100) / (1000 * s_p)))
 *      (the product stays below 2^47; sub_p <= s_p follows from the rank order).  Per secondary: mapq = 0, sub = 0, nsub = 0.
 *      Flags (u8).  Bit 0 is set for a primary, bit 1 for a KEPT chain.  A primary is always kept.  A secondary c with parent p is kept
 *      iff 100 * s_c >= pri_pct * s_p and fewer than best_n secondaries of p precede c in rank order -- what minimap2's -p and -N do.
 *      Per group: out_best[g] = the chain of rank 0, -1 for an empty group (an unmapped read).
 *      The formula is this project's own integer form of minimap2's mm_set_parent / mm_set_mapq.  It has the same ingredients -- the
 *      score gap to the best secondary, the anchor count, a score floor -- but it is not minimap2's float formula, and the results are
 *      not comparable number for number.
 *      Outputs per chain: out_parent (a chain number), out_rank, out_mapq, out_flag, out_sub, out_nsub; per group out_best (may be NULL;
 *      one entry with offsets == NULL).  All arrays live in the memory `where` names.  Host memory: staged, the call synchronises.
 *      Device memory: every kernel is queued on hip_stream and the call returns WITHOUT waiting for the stream -- it returns no count,
 *      so it needs no wait; its scratch comes from the pooled block and goes back from a host function queued behind the kernels (not
 *      capturable into a graph, as kh_chain_edits).
 *      KH_ERR_INVALID before anything is allocated, read or written: mask_pct > 100, pri_pct > 100, n_chains > 2^23 (the cap of
 *      kh_chain_ends), n_grp > n_chains + 2^24, n_grp == 0 with offsets given, `where` outside the enum, and while n_chains > 0 a null
 *      input or per-chain output.  n_chains == 0: KH_OK and every out_best entry = -1 (host memory: without a device).
 *      Offsets that do not ascend from 0 to n_chains: in host memory they are refused on the host, KH_ERR_INVALID with nothing written.
 *      In device memory nobody can see them before the kernels run: every group is clamped to [0, n_chains), nothing outside the
 *      arrays is touched, the outputs of the affected chains are unspecified and the status is KH_OK.  This is the price of not
 *      waiting. */
kh_status kh_chain_select(const uint32_t* q_start, const uint32_t* q_end, const int32_t* score, const uint32_t* count, uint64_t n_chains,
                          const uint64_t* offsets /* u64[n_grp+1] or NULL */, uint64_t n_grp,
                          uint32_t mask_pct, uint32_t pri_pct, uint32_t best_n, kh_mem where,
                          int32_t* out_parent, uint32_t* out_rank, uint8_t* out_mapq, uint8_t* out_flag, int32_t* out_sub, uint32_t* out_nsub /* each [n_chains] */,
                          int32_t* out_best /* [n_grp], [1] with offsets == NULL; may be NULL */, int device, void* hip_stream);

/* ---- one alignment record per chain.  The chain calls leave a read's alignment in pieces: one CSR row per anchor link
 *      (kh_chain_cigars), two rows and two clips per chain (kh_chain_ends), the intervals in the chains' first and last anchors.
 *      kh_chain_records joins them: per chain one row of runs -- the CIGAR of the whole read -- and the numbers of a PAF line.  It
 *      reads no text; it consumes only what the earlier calls wrote.
 *      Inputs: per anchor [m] qpos, rpos, rev and chain (the chain number of kh_chain_anchors, -1: none); the link CSR of
 *      kh_chain_cigars, lk_offsets [m + 1] and lk_ops [n_lk]; per chain [n_chains] c_first, c_last (anchor indices) and the read's byte
 *      interval [q_lo, q_hi); the ends of kh_chain_ends, e_q, e_r, e_clip [2 n_chains], en_offsets [2 n_chains + 1], en_ops [n_en];
 *      k (1..64) and ref_order (0 or 1).
 *      Rows of the two input CSRs.  Row i of a CSR with n runs is [a, b) with a = min(offsets[i], n), b = min(offsets[i + 1], n); it is
 *      EMPTY where b <= a or b - a > 63 (no row of the two calls is longer: 2 * 31 + 1).
 *      Members.  The members of chain c are the anchors i in [c_first[c], c_last[c]] with chain[i] == c; ascending anchor order is
 *      chain order (kh_chain_anchors: pred[i] < i).
 *      Validity.  out_valid[c] = 1 iff  c_first[c] <= c_last[c] < m;  chain[c_first[c]] == chain[c_last[c]] == c;
 *      q_lo <= qpos[first];  qpos[last] + k <= q_hi;  q_hi - q_lo < 2^28;  and every member but the first has a link row that is not
 *      empty (the condition under which the chain has a whole alignment at all).
 *      The row of a valid chain is the sequence of pieces, in read order:  S x (e_clip[2c] mod 2^28);  end row 2c (the head);  the link
 *      row of every member except the first, ascending;  k x '=' (the last seed);  end row 2c + 1 (the tail);
 *      S x (e_clip[2c + 1] mod 2^28)  -- fed run by run through this rule: a run of length 0 vanishes; a run whose op equals the op of
 *      the run before it adds its length to that run (mod 2^28, the width of the length field); any other run starts a new one.  Runs
 *      are (len << 4) | op in the BAM encoding (S = 4, I = 1, D = 2, '=' = 7, X = 8).  With ref_order == 1 the row of a chain whose
 *      bit 0 of rev[c_first[c]] is set is stored in the reverse run order, the orientation PAF and SAM expect; ref_order == 0 keeps
 *      read order.  An invalid chain has an empty row.
 *      Numbers per chain, all u32 with wrapping arithmetic.  Where the first two validity conditions hold, with f = c_first[c],
 *      l = c_last[c]:  qs = qpos[f] - e_q[2c] - q_lo  and  qe = qpos[l] + k + e_q[2c + 1] - q_lo, read-relative;
 *      rs = min(rpos[f], rpos[l]) - x  and  re = max(rpos[f], rpos[l]) + k + y  in reference coordinates, with (x, y) =
 *      (e_r[2c], e_r[2c + 1]) on the forward strand and (e_r[2c + 1], e_r[2c]) on the reverse strand (bit 0 of rev[f]): head and
 *      tail swap sides.  Elsewhere the four are 0.  qlen = q_hi - q_lo always.  For a valid chain n_match = the sum of its '=' runs,
 *      n_block = the sum of its '=', X, I and D runs, nm = the sum of its X, I and D runs; 0 for an invalid one.
 *      All arrays live in the memory `where` names.  out_ops == NULL: count only -- out_valid, the eight numbers, out_offsets
 *      [n_chains + 1] and *n_ops are written.  More runs than cap_ops: KH_ERR_INVALID with *n_ops set, the numbers and out_offsets
 *      written and out_ops untouched.  Device memory: everything is queued on hip_stream and the one host wait of a pass is the one
 *      that learns *n_ops.  Host memory: staged, the call synchronises.  Garbage in the arrays yields empty or wrong rows; no element
 *      outside the arrays is read or written.
 *      KH_ERR_INVALID before anything is allocated, read or written: k outside 1..64, ref_order > 1, m > 2^24, n_chains > 2^23, n_lk or
 *      n_en > 2^31, `where` outside the enum, a null out_offsets or n_ops, while n_chains > 0 a null chain array, end array or output
 *      (en_ops may be null while n_en == 0), and while both n_chains > 0 and m > 0 a null anchor array or link array (lk_ops may be
 *      null while n_lk == 0).  n_chains == 0: KH_OK, *n_ops = 0, out_offsets[0] = 0. */
kh_status kh_chain_records(const uint32_t* qpos /*[h|d] u32[m]*/, const uint32_t* rpos, const uint8_t* rev, const int32_t* chain, uint64_t m,
                           const uint64_t* lk_offsets /*[m+1]*/, const uint32_t* lk_ops /*[n_lk]*/, uint64_t n_lk,
                           const uint32_t* c_first, const uint32_t* c_last, const uint32_t* q_lo, const uint32_t* q_hi /* each [n_chains] */, uint64_t n_chains,
                           const uint32_t* e_q, const uint32_t* e_r, const uint32_t* e_clip /* each [2 n_chains] */,
                           const uint64_t* en_offsets /*[2 n_chains + 1]*/, const uint32_t* en_ops /*[n_en]*/, uint64_t n_en,
                           uint32_t k /*1..64*/, uint32_t ref_order /*0|1*/, kh_mem where,
                           uint8_t* out_valid, uint32_t* out_qs, uint32_t* out_qe, uint32_t* out_rs, uint32_t* out_re, uint32_t* out_qlen,
                           uint32_t* out_match, uint32_t* out_block, uint32_t* out_nm /* each [n_chains] */,
                           uint64_t* out_offsets /*[n_chains + 1]*/, uint32_t* out_ops /*[cap_ops] or NULL*/, uint64_t cap_ops, uint64_t* n_ops,
                           int device, void* hip_stream);

/* ---- a run CSR as CIGAR text.  Any (offsets [n_rows + 1], ops [n_ops]) pair of runs (len << 4) | op -- link rows, end rows, record
 *      rows -- becomes a byte CSR: row i is the ASCII of its runs, each the decimal length (1..9 digits: a length has 28 bits; 0 prints
 *      as "0") followed by the op letter from "MIDNSHP=X", '?' for the op codes 9..15.  No separator, no terminator.
 *      Bounds.  With o(i) = min(offsets[i], n_ops), base = o(0) and b(i) = max(o(i), base):  out_offsets[i] = the bytes of the runs
 *      [base, b(i)), and out_text holds the text of the runs [base, b(n_rows)) -- for offsets that ascend within [0, n_ops] exactly the
 *      rows' texts one after the other.  Offsets that descend give descending out_offsets; nothing outside the arrays is read or
 *      written.
 *      out_text == NULL: count only -- out_offsets and *n_text are written.  More bytes than cap_text: KH_ERR_INVALID with *n_text set,
 *      out_offsets written and out_text untouched.  Device memory: everything is queued on hip_stream, one host wait per pass to learn
 *      *n_text.  Host memory: staged, the call synchronises.
 *      KH_ERR_INVALID before anything is touched: n_rows or n_ops > 2^31, `where` outside the enum, a null out_offsets or n_text, a null
 *      offsets while n_rows > 0, a null ops while both n_rows > 0 and n_ops > 0.  n_rows == 0 or n_ops == 0: KH_OK, *n_text = 0, every
 *      out_offsets entry 0 (host memory: no device is needed). */
kh_status kh_cigar_text(const uint64_t* offsets /*[h|d] u64[n_rows+1]*/, uint64_t n_rows, const uint32_t* ops /*[h|d] u32[n_ops]*/, uint64_t n_ops, kh_mem where,
                        uint64_t* out_offsets /*[n_rows + 1]*/, uint8_t* out_text /*[cap_text] or NULL*/, uint64_t cap_text, uint64_t* n_text,
                        int device, void* hip_stream);

/* ---- anchors by target.  A reference of several sequences (contigs, chromosomes, transcripts) is indexed as ONE text in which the
 *      targets are separated by spacers of at least 32 bytes that are no base: a non-base byte matches nothing (kh_chain_edits), so a
 *      spacer costs at least 32 edits, more than max_edits can be (31) -- neither a chain link nor an end extension crosses one.  What
 *      is left is the chaining DP, which reads no text: kh_anchor_targets regroups the anchors of every segment (read) by the target
 *      they fall in, and the (segment, target) groups it returns are the segments to hand to kh_chain_anchors.  "Chains never cross a
 *      segment boundary" then reads "chains never cross a target".  Integers only.
 *      Inputs: the anchors qpos, rpos, rev [m] and the segment CSR seg_offsets [n_seg + 1] (NULL: one segment [0, m)) as
 *      kh_chain_anchors takes them; the target table t_start, t_end [n_t] -- target t covers the reference coordinates
 *      [t_start[t], t_end[t]), ascending and disjoint in a well-formed table; the seed length k.
 *      Target of an anchor.  With r = rpos[i]:
 *        lo = 0; hi = n_t; while (lo < hi) { mid = (lo + hi) >> 1; if (t_start[mid] <= r) lo = mid + 1; else hi = mid; }
 *      ub = lo (the plain upper bound of r in t_start) and t = ub - 1.  tid(i) = t iff t >= 0 and r < 2^31 and r + k <= t_end[t];
 *      otherwise tid(i) = KH_TARGET_NONE: the seed starts before every target, in a spacer, or runs over its target's end.  The table
 *      is not validated: an unsorted table gives the ids this loop gives, and never an access outside [0, n_t).
 *      Order.  Segment s is clamped as kh_chain_anchors clamps it: a = min(seg_offsets[s], m), b = max(a, min(seg_offsets[s + 1], m)).
 *      The output is the input sorted by (segment, tid, input index); KH_TARGET_NONE is the largest id, so those anchors stand last in
 *      their segment.  out_src[j] = the input index of output anchor j; out_q[j], out_r[j], out_v[j], out_tid[j] = qpos, rpos, rev
 *      and tid of that anchor, except that out_r[j] = KH_POS_INVALID where the id is KH_TARGET_NONE -- the DP never links such an
 *      anchor.  A segment whose anchors all have one id keeps its order: for a reference of one target the regrouping is the identity.
 *      Groups.  The groups are the maximal runs of equal (segment, tid) of the output, in order: group g is the output anchors
 *      [g_offsets[g], g_offsets[g + 1]) with g_offsets[0] = 0 and g_offsets[*n_grp] = m, g_seg[g] its segment and g_tid[g] its id
 *      (KH_TARGET_NONE for the group of the anchors without a target).  A segment without anchors has no group.  *n_grp <= m.
 *      All arrays live in the memory `where` names.  Device memory: every kernel is queued on hip_stream and the call waits once, to
 *      learn *n_grp.  Host memory: staged, the call synchronises.
 *      seg_offsets that do not ascend from 0 to m are seen on the device only: KH_ERR_INVALID after the kernels have run, with
 *      *n_grp = 0 and unspecified output contents; nothing outside the arrays is touched.
 *      KH_ERR_INVALID before anything is allocated, read or written: k outside 1..64, m > 2^24, n_t outside 1..2^24,
 *      n_seg > m + 2^24 or n_seg == 0 with seg_offsets given and m > 0, `where` outside the enum, a null g_offsets or n_grp, and while
 *      m > 0 a null input, table or output array.  m == 0: KH_OK, *n_grp = 0, g_offsets[0] = 0 (host memory: without a device).
 *      Route (kh_kernels_targets.h): one lane per anchor searches the table -- staged in LDS once per workgroup while
 *      n_t <= KH_TARGETS_STAGED_MAX (8192 targets: 64 KiB), through L2 beyond; then one wavefront per segment takes the smallest
 *      unplaced id, ballots the lanes that hold it and places them behind the running offset, one step per distinct id -- run twice,
 *      to count the groups and to write. */
#define KH_TARGET_NONE 0xFFFFFFFFu
#define KH_TARGETS_STAGED_MAX 8192u
kh_status kh_anchor_targets(const uint32_t* qpos /*[h|d] u32[m]*/, const uint32_t* rpos, const uint8_t* rev, uint64_t m,
                            const uint64_t* seg_offsets /*[n_seg+1] or NULL: one segment*/, uint64_t n_seg,
                            const uint32_t* t_start, const uint32_t* t_end /* each [n_t] */, uint64_t n_t, uint32_t k /*1..64*/, kh_mem where,
                            uint32_t* out_q, uint32_t* out_r, uint8_t* out_v, uint32_t* out_tid, uint32_t* out_src /* each [m] */,
                            uint64_t* g_offsets /*[m+1]*/, uint32_t* g_seg /*[m]*/, uint32_t* g_tid /*[m]*/, uint64_t* n_grp,
                            int device, void* hip_stream);

/* ---- the difference strings of alignment records.  The CIGAR of a record (kh_chain_records) says where its X, I and D runs are;
 *      kh_record_diffs reads the two texts and says which bases they were: per row the short cs string (minimap2's cs:Z:) or the MD
 *      string of SAM (MD:Z:).
 *      Inputs: the two texts as kh_chain_edits takes them -- rtext covers the reference coordinates [ref_base, ref_base + nr); a run
 *      CSR offsets [n_rows + 1], ops [n_ops] in the encoding of kh_chain_records, IN REFERENCE ORDER (the rows ref_order = 1 gives);
 *      per row [n_rows]: valid (ChainRecords), rev (bit 0: the strand), the read's byte interval [q_lo, q_hi) as kh_chain_records
 *      took it, and rs, the record's reference start.
 *      Bases.  The code of a byte is that of kh_chain_edits: A/a = 0, C/c = 1, G/g = 2, T/t = 3, any other byte 4.  With
 *      L = q_hi - q_lo the ORIENTED READ O of a row is  O[j] = code(qtext[q_lo + j])  on the forward strand and, with
 *      c = code(qtext[q_hi - 1 - j]),  O[j] = 3 - c if c < 4, else 4  on the reverse strand.  R[r] = code(rtext[r - ref_base]).
 *      The walk.  Row c is the runs [a, b), a = min(offsets[c], n_ops), b = min(offsets[c + 1], n_ops).  Cursors j = 0, r = rs[c]; the
 *      runs in order; a run of length 0 is skipped (whatever its op); otherwise with l its length:  S (4): j += l;  '=' (7) consumes l
 *      of both;  X (8) consumes l of both, base by base;  I (1) consumes l of O;  D (2) consumes l of R;  any other op code spoils the
 *      row.
 *      out_ok[c] = 1 iff  valid[c] != 0;  b > a;  q_lo <= q_hi <= nq;  no run spoils the row;  the walk ends with j = L;  every
 *      reference base the walk consumes lies in [ref_base, ref_base + nr)  -- all sums in 64 bits -- and the row's text is shorter
 *      than 2^32 bytes (no such text fits texts of at most 2^32 bases but one of X runs alone in cs).  Any other row has out_ok = 0
 *      and an empty text.
 *      KH_DIFF_CS, run by run:  '=' -> ':' and the decimal l;  X -> per base '*', "acgtn"[R], "acgtn"[O];  I -> '+' and l letters of
 *      O;  D -> '-' and l letters of R;  S -> nothing.  A row of S runs alone is ok and empty.
 *      KH_DIFF_MD keeps a counter n = 0 (u32, wrapping):  '=' adds l to n;  X -> per base the decimal n, "ACGTN"[R], n = 0;
 *      D -> the decimal n, '^', l letters of R, n = 0;  I and S print nothing and leave n alone;  after the last run the decimal n.
 *      So a row that starts or ends with an edit starts or ends with "0", two neighbouring edits have "0" between them, the matches on
 *      both sides of an insertion make one number, and the text matches [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*.
 *      Output: a byte CSR, out_offsets [n_rows + 1] and out_text, under the conventions of kh_cigar_text: out_text == NULL counts only
 *      -- out_ok, out_offsets and *n_text are written; more bytes than cap_text: KH_ERR_INVALID with *n_text set, out_ok and
 *      out_offsets written and out_text untouched.  Device memory: everything is queued on hip_stream, one host wait per pass to learn
 *      *n_text.  Host memory: staged, the call synchronises.  Garbage in any array yields empty or wrong rows; no element outside the
 *      arrays is read or written.
 *      KH_ERR_INVALID before anything is touched: kind > 1, n_rows or n_ops > 2^31, nq or nr > 2^32, `where` outside the enum, a null
 *      out_offsets or n_text, and while n_rows > 0 a null offsets, per-row array or out_ok, a null ops while n_ops > 0 and a null text
 *      of a length > 0.  n_rows == 0: KH_OK, *n_text = 0, out_offsets[0] = 0 (host memory: without a device).
 *      Route (kh_kernels_sam.h): one wavefront per row, 64 runs per step; wave prefix sums give every lane its cursors and its byte
 *      offset, a segmented wave sum the number in front of an MD edit; count, scan, emit. */
#define KH_DIFF_CS 0u
#define KH_DIFF_MD 1u
kh_status kh_record_diffs(const void* qtext /*[h|d]*/, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base,
                          const uint64_t* offsets /*[n_rows+1]*/, const uint32_t* ops /*[n_ops]*/, uint64_t n_ops,
                          const uint8_t* valid, const uint8_t* rev, const uint32_t* q_lo, const uint32_t* q_hi, const uint32_t* rs /* each [n_rows] */,
                          uint64_t n_rows, uint32_t kind /* KH_DIFF_CS | KH_DIFF_MD */, kh_mem where,
                          uint8_t* out_ok /*[n_rows]*/, uint64_t* out_offsets /*[n_rows+1]*/, uint8_t* out_text /*[cap_text] or NULL*/, uint64_t cap_text,
                          uint64_t* n_text, int device, void* hip_stream);

/* ---- byte ranges of a text as rows in reference orientation: SEQ and QUAL of SAM.  Row c is text[a, b) with a = min(lo[c], n) and
 *      b = min(hi[c], n), empty where b <= a.  Where bit 0 of rev[c] is clear the row is copied as it stands; where it is set it is
 *      copied back to front, and with complement == 1 every byte of such a row goes through A<->T, C<->G, a<->t, c<->g -- every other
 *      byte stays itself: N stays N, the case is kept.  complement == 0 reverses only (a quality string).
 *      Output: a byte CSR whose offsets are the prefix sums of the row lengths, under the conventions of kh_record_diffs (count only
 *      with out_text == NULL; KH_ERR_INVALID with *n_text set and out_offsets written when cap_text is too small; device memory:
 *      queued on hip_stream, one host wait per pass; host memory: staged).
 *      KH_ERR_INVALID before anything is touched: complement > 1, n_rows > 2^31, n > 2^32, `where` outside the enum, a null
 *      out_offsets or n_text, and while n_rows > 0 a null lo, hi or rev and a null text while n > 0.  n_rows == 0: KH_OK,
 *      *n_text = 0, out_offsets[0] = 0 (host memory: without a device).
 *      Route: one lane per row for the lengths, the index's scan, then one wavefront per row that moves 8-byte words: a reversed
 *      word is a byte swap and a SWAR complement. */
kh_status kh_oriented_rows(const void* text /*[h|d]*/, uint64_t n, const uint32_t* lo, const uint32_t* hi, const uint8_t* rev /* each [n_rows] */, uint64_t n_rows,
                           uint32_t complement /*0|1*/, kh_mem where,
                           uint64_t* out_offsets /*[n_rows+1]*/, uint8_t* out_text /*[cap_text] or NULL*/, uint64_t cap_text, uint64_t* n_text,
                           int device, void* hip_stream);

/* ---- paired reads.  The calls above map every read on its own; kh_pair_chains looks at the chain rows of the two mates of a fragment
 *      together: it picks the concordant combination, says whether the pair is proper, raises the quality of a mate that its partner
 *      pins to one copy of a repeat, and gives the template length.  Integers only: the kernel equals the model of tests/pair_model.py
 *      bit for bit.
 *      Inputs.  Per chain c of n_chains: the reference interval [rs[c], re[c]) (u32, global coordinates: ChainRecords rs / re), rev[c]
 *      (u8, bit 0: the strand), score[c] (i32, any value), tid[c] (u32 target number, KH_TARGET_NONE allowed; tid == NULL: all chains
 *      lie in one target), use[c] (u8, non-zero: the chain is a candidate; NULL: all are), mapq_in[c] (u8, the single-read quality;
 *      NULL: 0).  A CSR offsets [n_reads + 1] (required) gives the chains [offsets[s], offsets[s + 1]) of read s.  Reads 2p and 2p + 1
 *      are mate 1 and mate 2 of pair p; n_reads is even.  Parameters min_ins <= max_ins (u32, fragment length bounds) and unpaired_pen
 *      (u32).
 *      Candidates.  A chain TAKES PART if use says so and re > rs.  Of each mate only its KH_PAIR_CANDIDATES (64) best taking-part
 *      chains are candidates, in the CANDIDATE ORDER: score descending, ties to the smaller chain number.  A read with more kept loci
 *      is a repeat, whatever its partner says; the cap belongs to the definition (it bounds the work per pair), not to the kernel.
 *      A combination (a, b) -- a a candidate of mate 1, b one of mate 2 -- is CONCORDANT, for a forward-reverse library, iff
 *      tid[a] == tid[b] != KH_TARGET_NONE; bit 0 of rev[a] and rev[b] differ; with f the forward chain of the two and r the reverse
 *      one, rs_f <= rs_r and re_f <= re_r; and frag = re_r - rs_f lies in [min_ins, max_ins].  Its pair score is ps = s_a + s_b in
 *      signed 64-bit.  Combinations are ordered by ps descending, then a ascending, then b ascending (chain numbers); (a*, b*) is the
 *      first, ps* its score.
 *      Singles.  a0 and b0 are the first candidate of each mate in the candidate order, -1 for a mate without candidates.
 *      Proper.  Pair p is PROPER iff a concordant combination exists and ps* + unpaired_pen >= s_a0 + s_b0 (64-bit).  Its rows are then
 *      (a*, b*), otherwise (a0, b0).
 *      Quality.  For a proper pair and mate 1: alt1 = max(0, the greatest ps over the concordant combinations with a != a*), 0 if
 *      there is none; pq1 = 0 if ps* <= 0, else min(60, floor(60 * (ps* - alt1) / ps*)); out_mapq[2p] = max(mapq_in[a*], pq1).  Mate 2
 *      likewise over b != b*.  A pair that is not proper: out_mapq[s] = mapq_in[out_row[s]], 0 where the read has no row.
 *      Template length.  Where both mates have a row and the two rows share a target that is not KH_TARGET_NONE (tid == NULL: they
 *      always do): t = max(re) - min(rs) over the two rows, in 64-bit, clamped to 2^31 - 1; the mate whose rs is smaller gets +t, the
 *      other -t; equal rs: mate 1 gets +t.  Otherwise 0.
 *      Outputs.  Per read [n_reads]: out_row (i32, a chain number or -1), out_mapq (u8), out_tlen (i32).  Per pair [n_reads / 2]:
 *      out_flag (u8: bit 0 = proper, bit 1 = both mates have a row, bit 2 = the two rows share a target as above), out_score (i32: ps*
 *      clamped to the i32 range) and out_nconc (u32: the number of concordant combinations, at most 4096).
 *      Corners this text decides.  out_score and out_nconc describe the concordant combinations whether or not the pair is proper;
 *      both are 0 when there is none.  A chain with re <= rs never takes part, not even as a single.  The test of a combination
 *      compares the strand bits only: two chains of one target with the same strand, or reverse before forward, are never concordant,
 *      whatever their distance.  A mate whose candidates all have tid == KH_TARGET_NONE can have a row (its single) but no proper
 *      pair, bit 2 stays clear and its template length is 0.  The rows of a pair that is not proper may lie on one target: then bit 2 is
 *      set and the template length is given, the way SAM prints TLEN for a discordant pair on one reference.
 *      Conventions are those of kh_chain_select.  All arrays live in the memory `where` names.  Device memory: the kernel is queued on
 *      hip_stream and the call returns WITHOUT waiting for the stream (it returns no count); the staging block of a host call comes
 *      from the pooled block.  Host memory: staged, the call synchronises.
 *      KH_ERR_INVALID before anything is allocated, read or written: odd n_reads, min_ins > max_ins, n_chains > 2^23,
 *      n_reads > n_chains + 2^24, `where` outside the enum, a null offsets, while n_reads > 0 a null per-read or per-pair output, and
 *      while n_chains > 0 a null rs, re, rev or score.  n_reads == 0: KH_OK, nothing written.  n_chains == 0: every out_row entry -1 and
 *      every other output 0 (host memory: without a device).
 *      Offsets that do not ascend from 0 to n_chains: in host memory they are refused on the host, KH_ERR_INVALID with nothing written
 *      (n_reads == 0 included: offsets[0] must be 0 = n_chains).  In device memory nobody can see them before the kernel runs: every
 *      group is clamped to [0, n_chains], nothing outside the arrays is touched, the outputs of the affected pairs are unspecified and
 *      the status is KH_OK.
 *      Route (kh_kernels_pair.h): one wavefront per pair, no LDS, no scratch, no atomics.  A mate's candidates are streamed 64 chains
 *      at a time -- rank by counting, push into order, the lane-wise larger of the kept 64 and the reversed chunk (half a bitonic
 *      merge), rank and push again; a group of at most 64 chains is one load -- then lane i holds candidate i of mate 1, a uniform loop
 *      broadcasts those of mate 2, and (a*, b*) is one wave max over a packed 64-bit key.
 *      Not here: an insert-size distribution, other library orientations.  A mate that has no row at all is kh_mate_rescue's
 *      (below); re-pairing a mate whose own rows are all discordant is not done anywhere. */
#define KH_PAIR_CANDIDATES 64u
kh_status kh_pair_chains(const uint32_t* rs /*[h|d] u32[n_chains]*/, const uint32_t* re, const uint8_t* rev, const int32_t* score,
                         const uint32_t* tid /* or NULL */, const uint8_t* use /* or NULL */, const uint8_t* mapq_in /* or NULL */, uint64_t n_chains,
                         const uint64_t* offsets /* u64[n_reads+1] */, uint64_t n_reads /* even */,
                         uint32_t min_ins, uint32_t max_ins, uint32_t unpaired_pen, kh_mem where,
                         int32_t* out_row, uint8_t* out_mapq, int32_t* out_tlen /* each [n_reads] */,
                         uint8_t* out_flag, int32_t* out_score, uint32_t* out_nconc /* each [n_reads / 2] */, int device, void* hip_stream);

/* ---- mate rescue.  kh_pair_chains only looks at rows that seeding found.  A mate whose seeds were all destroyed (errors every dozen
 *      bases, a variant cluster) or masked (drop_above) has no row, although its partner says to within max_ins bases where it must
 *      lie.  kh_mate_rescue aligns such a mate END TO END inside a window of the reference: where it ends, at what distance, where it
 *      starts and by which operations.  There is no seed, so the first phase scans the whole window; the second is the extension of
 *      kh_chain_ends run backwards from the end the scan found.  Integers only: the kernels equal tests/rescue_model.py bit for bit.
 *      Inputs.  The two texts with ref_base as for kh_chain_ends; bases and the match rule are those of kh_chain_edits (an N matches
 *      nothing, another N included); max_edits 0..31.  Per request j of n: q_lo[j], q_hi[j] (u32) -- the mate is qtext[q_lo, q_hi),
 *      m = q_hi - q_lo; w_lo[j], w_hi[j] (u32) -- the window in global reference coordinates, rtext[w_lo - ref_base, w_hi - ref_base),
 *      W = w_hi - w_lo; rev[j] (u8) -- bit 0 is the strand on which the mate is expected.
 *      Pattern.  R = the mate as it stands if rev is 0, its reverse complement if 1.  Everything below is in reference order, like
 *      ChainRecords with ref_order.
 *      Which requests are looked at.  out_edits[j] = KH_RESCUE_NONE (-1), all other numbers 0 and an empty row unless
 *      q_lo < q_hi <= nq; 1 <= m <= KH_RESCUE_MAX_READ (512); ref_base <= w_lo <= w_hi; w_hi - ref_base <= nr; and
 *      W <= KH_RESCUE_MAX_WINDOW (65536).  Garbage therefore yields -1 or wrong rows; it never causes a read outside the texts or a
 *      write outside the arrays.
 *      Phase 1, the scan.  D is the unit-cost edit matrix of R (rows 0..m) against the window (columns 0..W) with a free reference
 *      start: D[0][c] = 0 for every c, D[i][0] = i, D[i][c] = min(D[i-1][c-1] + (R[i-1] does not match window base c-1), D[i-1][c] + 1,
 *      D[i][c-1] + 1).  d* = min over c of D[m][c]; e = the smallest c attaining d*, last = the greatest.  d* > max_edits:
 *      out_edits[j] = KH_RESCUE_OVER (-2), all other numbers 0 and an empty row.
 *      Phase 2, start and operations: the extension of kh_chain_ends, word for word, for a HEAD.  A = R read downwards from its last
 *      base, n = m; B = the reference read downwards from window column e - 1, |B| = min(m + max_edits, e), so B never leaves the
 *      window.  Diagonals, hi(d), the candidates X / I / D, "dropped, not clamped" and the move rule are as defined there.  One
 *      difference: the alignment never stops early and there is no clip cost -- the target is the first level E <= max_edits at which
 *      some diagonal holds n; among the diagonals that hold n at level E the smaller |d| wins, then d < 0.  (That is the extension
 *      with clip_cost 0: S = F.)  E EQUALS d* BY CONSTRUCTION: an alignment of all of R that ends at column e costs D[m][e] = d* at
 *      the least, and the one that attains it uses at most m + d* reference bases and stays within |d| <= d*.  The traceback from
 *      that point to (0, 0), stored in the reverse of the order found, is the row: the row is in reference order.
 *      Outputs per request: out_edits (i32: d*, -1 or -2); out_rs, out_re (u32, global: re = w_lo + e, rs = re - (n + d));
 *      out_span (u32: last - e) -- an ambiguity measure: ends tied within d* columns are one placement with its gaps shifted, a larger
 *      span means a second placement inside the window; and a CSR out_offsets [n + 1] / out_ops in the BAM run encoding of
 *      kh_chain_cigars (=, X, I, D; no S).  Adjacent runs never share an op; a row has at most 2 d* + 1 <= 63 runs, consumes exactly
 *      m bases of R and re - rs reference bases and has d* edit bases.
 *      Mapping quality.  The call gives none.  The rule of the SAM writer (write_sam_rescued) is: a rescued mate takes the pair
 *      quality of its partner if out_span <= out_edits, else 0.
 *      Conventions are those of kh_chain_ends.  All arrays live in the memory `where` names.  out_ops == NULL: count only -- the four
 *      numbers, out_offsets and *n_ops are written.  More runs than cap_ops: KH_ERR_INVALID with *n_ops set, the numbers and
 *      out_offsets written and out_ops untouched.  Device memory: everything is queued on hip_stream and the one host wait is the one
 *      that learns *n_ops.  Host memory: staged, the call synchronises.
 *      KH_ERR_INVALID before anything is allocated, read or written: max_edits > 31, n > 2^24, nq >= 2^31, ref_base + nr > 2^31,
 *      `where` outside the enum, a null out_offsets or n_ops, and while n > 0 a null array, a null output or a null text of positive
 *      length.  n == 0: KH_OK, *n_ops = 0, out_offsets[0] = 0.
 *      Route (kh_kernels_rescue.h): phase 1 is one LANE per request, Myers' bit-vector recurrence in Hyyro's block form over
 *      ceil(m / 64) words with the pattern as three bit planes, all in registers, instantiated by word count; phase 2 one wavefront
 *      per request that phase 1 settled, through the device functions of kh_chain_ends; then the one count-scan-emit tail.
 *      Not here: soft clips in a rescued alignment, a mate with a discordant row of its own, other library orientations. */
#define KH_RESCUE_NONE (-1)
#define KH_RESCUE_OVER (-2)
#define KH_RESCUE_MAX_READ 512u
#define KH_RESCUE_MAX_WINDOW 65536u
kh_status kh_mate_rescue(const void* qtext /*[h|d] u8[nq]*/, uint64_t nq, const void* rtext /*[h|d] u8[nr]*/, uint64_t nr, uint32_t ref_base,
                         const uint32_t* q_lo /*[h|d] u32[n]*/, const uint32_t* q_hi, const uint32_t* w_lo, const uint32_t* w_hi,
                         const uint8_t* rev /*[h|d] u8[n]*/, uint64_t n, uint32_t max_edits /*0..31*/, kh_mem where,
                         int32_t* out_edits, uint32_t* out_rs, uint32_t* out_re, uint32_t* out_span /* each [n] */,
                         uint64_t* out_offsets /*[n + 1]*/, uint32_t* out_ops /*[cap_ops] or NULL*/, uint64_t cap_ops, uint64_t* n_ops,
                         int device, void* hip_stream);

/* ---- SAM lines from line columns.  Everything a SAM alignment line is made of already exists as columns and byte CSRs (the read and
 *      target names, kh_cigar_text, kh_oriented_rows, kh_record_diffs); kh_sam_lines turns n_lines rows of LINE COLUMNS into the text
 *      of the lines.  It knows nothing of mappings or pairs: which line prints what is the caller's (sam.sam_line_columns), so one
 *      call serves unpaired and paired output.  The kernels equal tests/samtext_model.py byte for byte.
 *      Byte CSRs.  Seven of them, each four arguments: X_off (u64 [n_X + 1]), X_text (u8 [X_bytes]), the number of rows n_X and the
 *      number of bytes X_bytes: names (read names), tnames (target names), cigar (CIGAR text), seq (SEQ rows), qual (QUAL rows), md
 *      and cs (difference strings).  Any of them may be absent: n_X == 0 (then X_off and X_text may be null and are not read).
 *      ROW r of a CSR: r is INSIDE iff 0 <= r < n_X; its bytes are X_text[a, b) with a = min(X_off[r], X_bytes) and
 *      b = min(X_off[r + 1], X_bytes), EMPTY where b <= a.  A row index outside its CSR is never an access: what it prints is said
 *      per field below.
 *      Line columns, each [n_lines]: l_name, l_rname, l_cigar, l_rnext, l_seq, l_qual, l_md, l_cs (i32 row indexes into names,
 *      tnames, cigar, tnames, seq, qual, md, cs); l_flag, l_pos, l_pnext, l_nm, l_cm (u32); l_tlen, l_s1, l_s2 (i32); l_mapq (u8);
 *      l_tp (u8, one byte printed as it is); l_tags (u8, a mask of KH_SAMTAG_*).
 *      Line i is, with TAB between the fields and no TAB at its end:
 *        QNAME   row l_name[i] of names; '*' where the row is outside (an empty row prints nothing)
 *        FLAG    l_flag[i]
 *        RNAME   row l_rname[i] of tnames; '*' where outside (-1 is the way to say so)
 *        POS     l_pos[i]
 *        MAPQ    l_mapq[i]
 *        CIGAR   row l_cigar[i] of cigar; '*' where outside
 *        RNEXT   '=' where l_rnext[i] == KH_SAM_RNEXT_SAME (-2); else row l_rnext[i] of tnames; '*' where outside
 *        PNEXT   l_pnext[i]
 *        TLEN    l_tlen[i]
 *        SEQ     row l_seq[i] of seq; '*' where the row is outside OR empty
 *        QUAL    row l_qual[i] of qual; '*' where the row is outside OR empty
 *      then, each with a TAB in front and only where its bit of l_tags[i] is set (the bits are independent; bits 4..7 are ignored):
 *        KH_SAMTAG_BASE (1)   NM:i:<l_nm[i]>  tp:A:<the byte l_tp[i]>  cm:i:<l_cm[i]>  s1:i:<l_s1[i]>
 *        KH_SAMTAG_S2 (2)     s2:i:<l_s2[i]>
 *        KH_SAMTAG_MD (4)     MD:Z:<row l_md[i] of md; nothing where the row is outside>
 *        KH_SAMTAG_CS (8)     cs:Z:<row l_cs[i] of cs; nothing where the row is outside>
 *      and one line feed (10).  l_tags[i] == 0 gives exactly the 11 mandatory fields: the line of an unmapped read.  Numbers are
 *      decimal without padding, a '-' in front of a negative one: what "%d" prints.
 *      Output: a byte CSR -- out_offsets [n_lines + 1], the prefix sums of the line lengths, and out_text, the lines one after the
 *      other -- under the conventions of kh_cigar_text: out_text == NULL counts only (out_offsets and *n_text are written); more
 *      bytes than cap_text: KH_ERR_INVALID with *n_text set, out_offsets written and out_text untouched.  All arrays live in the
 *      memory `where` names.  Device memory: everything is queued on hip_stream, one host wait per pass to learn *n_text.  Host
 *      memory: staged, the call synchronises.
 *      A line is shorter than 2^32 bytes because the call is: KH_ERR_INVALID unless
 *      names_bytes + 2 tnames_bytes + cigar_bytes + seq_bytes + qual_bytes + md_bytes + cs_bytes + KH_SAM_LINE_FIXED < 2^32
 *      (KH_SAM_LINE_FIXED = 256 bounds the separators, numbers and tag names of a line; a line can print a target name twice).
 *      KH_ERR_INVALID before anything is allocated, read or written: that sum, n_lines or any n_X > 2^31, any X_bytes > 2^32, `where`
 *      outside the enum, a null out_offsets or n_text, a null X_off while n_X > 0, a null X_text while X_bytes > 0, and a null line
 *      column while n_lines > 0 (all nineteen are needed, whatever the masks say).  n_lines == 0: KH_OK, *n_text = 0,
 *      out_offsets[0] = 0 (host memory: without a device).
 *      Route (kh_kernels_samtext.h): both passes are one wavefront per line in which lane p sizes piece p (a field with the literal in
 *      front of it) through one device function.  The count pass adds the sizes up by a wave sum -- row lengths and digit counts, no
 *      text is read --; the index's scan makes the offsets; the emit pass places the pieces by a wave prefix sum, every lane writes
 *      its own literal and digits and the wave copies the CSR rows in 8-byte words aligned to the destination. */
#define KH_SAMTAG_BASE 1u
#define KH_SAMTAG_S2 2u
#define KH_SAMTAG_MD 4u
#define KH_SAMTAG_CS 8u
#define KH_SAM_RNEXT_SAME (-2)
#define KH_SAM_LINE_FIXED 256u
kh_status kh_sam_lines(const uint64_t* names_off /*[h|d] u64[n_names+1]*/, const uint8_t* names_text /*[h|d] u8[names_bytes]*/, uint64_t n_names, uint64_t names_bytes,
                       const uint64_t* tnames_off, const uint8_t* tnames_text, uint64_t n_tnames, uint64_t tnames_bytes,
                       const uint64_t* cigar_off, const uint8_t* cigar_text, uint64_t n_cigar, uint64_t cigar_bytes,
                       const uint64_t* seq_off, const uint8_t* seq_text, uint64_t n_seq, uint64_t seq_bytes,
                       const uint64_t* qual_off, const uint8_t* qual_text, uint64_t n_qual, uint64_t qual_bytes,
                       const uint64_t* md_off, const uint8_t* md_text, uint64_t n_md, uint64_t md_bytes,
                       const uint64_t* cs_off, const uint8_t* cs_text, uint64_t n_cs, uint64_t cs_bytes,
                       const int32_t* l_name /*[h|d] each [n_lines]*/, const uint32_t* l_flag, const int32_t* l_rname, const uint32_t* l_pos, const uint8_t* l_mapq,
                       const int32_t* l_cigar, const int32_t* l_rnext, const uint32_t* l_pnext, const int32_t* l_tlen, const int32_t* l_seq, const int32_t* l_qual,
                       const uint8_t* l_tags, const uint32_t* l_nm, const uint8_t* l_tp, const uint32_t* l_cm, const int32_t* l_s1, const int32_t* l_s2,
                       const int32_t* l_md, const int32_t* l_cs, uint64_t n_lines, kh_mem where,
                       uint64_t* out_offsets /*[n_lines+1]*/, uint8_t* out_text /*[cap_text] or NULL*/, uint64_t cap_text, uint64_t* n_text,
                       int device, void* hip_stream);

/* ---- FASTQ records.  The mapper calls take (seq, read_starts, read_ends) and the SAM writers read names and a quality text laid out
 *      like seq; kh_fastq_records finds where those are in the text of a FASTQ file and kh_pack_rows (below) gathers them, so the input
 *      side needs no loop over reads on the host (fastq.read_fastq).  The kernels equal tests/fastq_model.py bit for bit.
 *      Lines.  The line number of a byte is the number of '\n' (10) before it: the rule of kh_kmers_from_fastq.  Line j runs from after
 *      newline j - 1 (line 0: from byte 0) up to, not including, newline j; a non-empty remainder after the last newline is a last line
 *      that ends at n.  One '\r' (13) directly before the end of a line is not part of the line.  Multi-line records are not known.
 *      Records.  Record r is lines 4r .. 4r + 3; *n_records = (number of lines) / 4; *tail_lines = the number of NON-EMPTY lines among
 *      the up to three left over, 0..3 (one trailing blank line is harmless, lines of a record cut short are not).
 *      Columns of record r, byte offsets into text:
 *        [seq_lo, seq_hi)   line 4r + 1
 *        qual_lo            the start of line 4r + 3 (the quality of base seq_lo + i is the byte qual_lo + i)
 *        name_lo            the start of line 4r, plus 1 if that byte is '@'
 *        name_hi            the first byte <= 0x20 (a blank, a tab: the comment begins) at or after name_lo, or the line's end
 *      With KH_FASTQ_STRIP_MATE in flags: a name longer than 2 bytes that ends in "/1" or "/2" loses those two bytes (name_hi -= 2), so
 *      the two mates of a pair carry one name; the name "/1" itself stays.
 *      status[r] is a set of bits: KH_FASTQ_NO_AT (1) line 4r does not begin with '@'; KH_FASTQ_NO_PLUS (2) line 4r + 2 does not begin
 *      with '+'; KH_FASTQ_LENGTHS (4) line 4r + 3 is not as long as line 4r + 1; KH_FASTQ_NO_NAME (8) the name is empty.  A record with
 *      a status other than 0 is KEPT, so that every later record -- and a mate in a second file -- keeps its number, as an EMPTY read:
 *      seq_hi = seq_lo and qual_lo = seq_lo (the name columns are as defined above).  *n_bad counts such records.
 *      Count, then emit.  With the five columns NULL the call counts: only *n_records, *n_bad and *tail_lines are written (status and cap
 *      are not looked at).  With the five columns given cap entries each (status: cap entries or NULL) cap must be >= the record count:
 *      then entries [0, *n_records) of every column are written and no other; else KH_ERR_INVALID with *n_records set and nothing else
 *      written.  n_bad and tail_lines may be NULL.  The text, the columns and status live in the memory `where` names; the three counts
 *      are host variables.  Device memory: everything is queued on hip_stream, one host wait per call to learn the counts.  Host memory:
 *      staged, the call synchronises.  The text may start at any byte: 8-byte loads where it is 8-byte aligned, bytes otherwise.
 *      KH_ERR_INVALID before anything is allocated, read or written: n >= 2^32, a flag bit other than KH_FASTQ_STRIP_MATE, `where`
 *      outside the enum, a NULL n_records, a NULL text while n > 0, some but not all of the five columns NULL.  n == 0: KH_OK and three
 *      zeros, without a device.
 *      Route (kh_kernels_fastq.h): k_newline_tile_sums and the scan of kh_kmers_from_fastq give every 2048-byte tile its first line;
 *      k_fastq_line_ends writes the offset of every newline; k_fastq_records, a lane per record, reads five neighbouring line ends.  The
 *      scratch holds one u32 per possible line: n of them in the count pass, 4 cap + 4 in the emit pass. */
#define KH_FASTQ_STRIP_MATE 1u
#define KH_FASTQ_NO_AT 1u
#define KH_FASTQ_NO_PLUS 2u
#define KH_FASTQ_LENGTHS 4u
#define KH_FASTQ_NO_NAME 8u
kh_status kh_fastq_records(const void* text /*[h|d] u8[n]*/, uint64_t n, uint32_t flags, kh_mem where,
                           uint32_t* name_lo, uint32_t* name_hi, uint32_t* seq_lo, uint32_t* seq_hi, uint32_t* qual_lo /*[h|d] u32[cap], or all NULL*/,
                           uint8_t* status /*[h|d] u8[cap] or NULL*/, uint64_t cap,
                           uint64_t* n_records, uint64_t* n_bad, uint32_t* tail_lines, int device, void* hip_stream);

/* ---- byte rows gathered to given places: out[dst[i] + j] = text[lo[i] + j] for j < len_i = hi[i] - lo[i], and with sep >= 0 also
 *      out[dst[i] + len_i] = sep (behind EVERY row, an empty one too).  A row that is not inside the text -- hi[i] < lo[i] or
 *      hi[i] > n -- is an empty row.  Every store is clamped to out_n: a byte that would land at or beyond it is dropped.  Bytes of
 *      out that no row and no separator covers are not written, so several calls can fill one buffer (two files interleaved: the rows of
 *      the first at the even places, of the second at the odd ones).  Keeping the destinations disjoint is the caller's: rows that
 *      overlap leave unspecified bytes of theirs inside out, never a stray access.  This is the copy of kh_oriented_rows without its
 *      CSR: the caller says where a row goes (fastq.read_fastq: cumulative sums of the lengths).
 *      All arrays live in the memory `where` names.  Device memory: the one kernel (one wavefront per row, 8-byte words aligned to
 *      the destination, 64 per step) is queued on hip_stream and the call does not wait.  Host memory: staged -- out is copied in and
 *      back --, the call synchronises.
 *      KH_ERR_INVALID before anything is read or written: n or out_n >= 2^32, n_rows > 2^31, sep outside -1..255, `where` outside
 *      the enum, and with n_rows > 0 a NULL lo, hi or dst, a NULL text while n > 0, a NULL out while out_n > 0. */
kh_status kh_pack_rows(const void* text /*[h|d] u8[n]*/, uint64_t n, const uint32_t* lo, const uint32_t* hi, const uint64_t* dst /*[h|d] [n_rows]*/, uint64_t n_rows,
                       int sep /* -1: none, 0..255: written behind every row */, kh_mem where, uint8_t* out /*[h|d] u8[out_n]*/, uint64_t out_n,
                       int device, void* hip_stream);

/* freed table buffers and workspaces are cached per device for reuse; this returns them to the driver */
kh_status kh_release_cached_memory(int device);

const char* kh_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KMERHASH_AMD_H_ */
