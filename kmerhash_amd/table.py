"""Host-side mirror of the reference's table interface over the C-ABI (include/kmerhash_amd.h).

Class and member names follow the reference (fsc::hashmap_robinhood_doubling, hashmap_robinhood.hpp:124-126;
fsc::hashmap_linearprobe_doubling, hashmap_linearprobe.hpp:96-98): insert / find / count / erase / update /
size / capacity / reserve / rehash / clear / to_vector / keys / set_{min,max}_load_factor.

Batches are numpy arrays (host memory, copied by the library) or torch CUDA tensors (device memory, zero
copy; int64/uint64 keys, int32/uint32 values).  Results come back in the same kind of container.
torch is plumbing only (device buffers + the current stream); all work happens in libkmerhash_amd.so.
There is no CPU fallback: constructing a table without the HIP library or without a GPU raises.
"""
import ctypes as C

import numpy as np

from . import _capi as K
from ._call import HOST, _Buf, _Handle, alloc, check, check_same, stream_of, torch  # noqa: F401  (torch: imported from here by other modules)
from ._capi import (KH_HASH_FARM64, KH_HASH_IDENTITY, KH_HASH_MURMUR3_X64_128_H0, KH_HASH_MURMUR3_X86_128_LO64,
                    KH_KIND_LINEARPROBE, KH_KIND_ROBINHOOD, KhError, KhLogicError, KhRetry)  # noqa: F401

HASHES = {
    "identity": KH_HASH_IDENTITY,
    "murmur3avx64": KH_HASH_MURMUR3_X86_128_LO64,   # fsc::hash::murmur3avx64 == murmur_x86
    "murmur_x86": KH_HASH_MURMUR3_X86_128_LO64,
    "murmur": KH_HASH_MURMUR3_X64_128_H0,           # fsc::hash::murmur (x64_128, h[0])
    "farm": KH_HASH_FARM64,
}


def _hash_id(h):
    return HASHES[h] if isinstance(h, str) else int(h)


class _TableCore(_Handle):
    """handle + scalar state of a table of either key width over the C-ABI entry points PREFIX + name; no batch members"""
    PREFIX = "kh_"
    STATUS_ERRORS = {K.KH_ERR_FULL: KhLogicError, K.KH_ERR_RETRY: KhRetry}
    KIND = None
    DEFAULT_MIN_LF = None
    DEFAULT_MAX_LF = None

    def __init__(self, capacity=128, min_load_factor=None, max_load_factor=None, hash="murmur3avx64", seed=43, device=0):
        self.device = int(device)
        mn = self.DEFAULT_MIN_LF if min_load_factor is None else min_load_factor
        mx = self.DEFAULT_MAX_LF if max_load_factor is None else max_load_factor
        widths = (8, 4) if self.WORDS == 1 else ()      # kh_create takes the key / value widths, kh_wide_create has them fixed
        self._create(self.KIND, *widths, _hash_id(hash), seed, capacity, mn, mx, self.device)

    def _kv(self, keys, vals, msg="keys/vals must have equal length and live in the same memory space", memory_msg=None):
        """the key batch and the optional value batch of one call, checked, the current stream adopted -> (kb, vb, pointer to the values)"""
        kb = _Buf.keys(keys, self.WORDS)
        vb = None if vals is None else _Buf(vals, np.uint32)
        if memory_msg is not None:          # (a caller that says which of the two it was)
            check_same(msg, kb, vb, memory=False)
            msg = memory_msg
        check_same(msg, kb, vb)
        self._adopt_stream(kb, vb)
        return kb, vb, None if vb is None else vb.ptr

    def _query(self, keys):
        """the key batch of a lookup or an erase, the current stream adopted"""
        kb = _Buf.keys(keys, self.WORDS)
        self._adopt_stream(kb)
        return kb

    # -- scalar state ------------------------------------------------------------------------------
    def size(self):
        return self._scalar("size")

    def __len__(self):
        return self.size()

    def capacity(self):
        return self._scalar("capacity")

    def set_min_load_factor(self, f):
        self._chk(self._fn("set_min_load_factor")(self._h, f))

    def set_max_load_factor(self, f):
        self._chk(self._fn("set_max_load_factor")(self._h, f))

    def _lf(self, i):
        f = [C.c_float(), C.c_float(), C.c_float()]
        self._chk(self._fn("get_load_factors")(self._h, C.byref(f[0]), C.byref(f[1]), C.byref(f[2])))
        return f[i].value

    def get_min_load_factor(self):
        return self._lf(0)

    def get_max_load_factor(self):
        return self._lf(1)

    def get_load_factor(self):
        return self._lf(2)

    def clear(self):
        self._chk(self._fn("clear")(self._h))

    def reserve(self, n):
        self._chk(self._fn("reserve")(self._h, int(n)))

    def rehash(self, b):
        self._chk(self._fn("rehash")(self._h, int(b)))

    def displacement_histogram(self):
        hist, ptr = alloc(HOST, 128, np.uint64)
        self._chk(self._fn("displacement_histogram")(self._h, ptr))
        return hist

    def export_info(self):
        info, ptr = alloc(HOST, self.capacity(), np.uint8)
        self._chk(self._fn("export_info")(self._h, ptr))
        return info

    # -- value-range operations: the elements with lo <= value <= hi (unsigned 32-bit), one pass over the slots on the GPU ---------
    @staticmethod
    def _value_range(lo, hi):
        lo, hi = int(lo), int(hi)
        if not (0 <= lo <= 0xFFFFFFFF and 0 <= hi <= 0xFFFFFFFF):
            raise ValueError("value range bounds must be unsigned 32-bit integers, got [%d, %d]" % (lo, hi))
        return lo, hi

    def value_histogram(self, nbins=256):
        """uint64[nbins]: out[b] = number of elements with value b, the last bin those with value >= nbins - 1 (nbins 1..16384).
        On a k-mer counter this is the k-mer spectrum."""
        nbins = int(nbins)
        hist, ptr = alloc(HOST, min(max(nbins, 1), 16384), np.uint64)
        self._chk(self._fn("value_histogram")(self._h, nbins if 0 <= nbins <= 0xFFFFFFFF else 0, ptr))      # (0: refused by the library)
        return hist

    def count_values(self, lo, hi):
        """number of elements with lo <= value <= hi (lo > hi: the empty range)"""
        lo, hi = self._value_range(lo, hi)
        n = C.c_uint64()
        self._chk(self._fn("select_values")(self._h, lo, hi, K.KH_MEM_HOST, None, None, 0, C.byref(n)))
        return n.value

    def select_values(self, lo, hi, device=False):
        """(keys, vals) of the elements with lo <= value <= hi in slot order (the order of to_vector()): numpy arrays, or CUDA
        tensors (int64 keys, int32 values: the bit patterns) written on the GPU when device=True.  A table of 16-byte keys returns
        (m, 2) keys.  select_values(0, 0xFFFFFFFF, device=True) is to_vector() into device memory."""
        lo, hi = self._value_range(lo, hi)
        m = self.size() if (lo, hi) == (0, 0xFFFFFFFF) else self.count_values(lo, hi)
        if device and torch is None:
            raise RuntimeError("select_values(device=True) needs torch")
        mem = _Buf.memory(self.device) if device else HOST
        keys, kptr = alloc(mem, m if self.WORDS == 1 else (m, self.WORDS), np.uint64, empty=True)
        vals, vptr = alloc(mem, m, np.uint32, empty=True)
        self._adopt_stream(mem)
        n = C.c_uint64()
        self._chk(self._fn("select_values")(self._h, lo, hi, mem.where, kptr, vptr, m, C.byref(n)))
        assert n.value == m, (n.value, m)
        return keys, vals

    def merge(self, other, op="plus"):
        """every (key, value) pair of `other` reduce-inserted into this table with `op` ("plus" | "min" | "max" | "or"): keys both
        hold get op(mine, theirs), the rest are inserted.  The pairs go from table to table in device memory (select_values over the
        whole value range, then insert_reduce); `other` is not changed.  Both tables must have the same key width.  Returns #new keys."""
        K.reduce_op(op)
        if not isinstance(other, _TableCore) or other.PREFIX != self.PREFIX:
            raise ValueError("merge: the tables differ in key width")
        keys, vals = other.select_values(0, 0xFFFFFFFF, device=True)
        if vals.numel() == 0:
            return 0
        if keys.device.index != self.device:
            keys, vals = keys.to("cuda:%d" % self.device), vals.to("cuda:%d" % self.device)
        return self.insert_reduce(keys, vals, op)

    def erase_values(self, lo, hi):
        """erases every element with lo <= value <= hi; the table afterwards is the table after erase() of exactly those keys.
        Returns the number erased."""
        lo, hi = self._value_range(lo, hi)
        n = C.c_uint64()
        self._chk(self._fn("erase_values")(self._h, lo, hi, C.byref(n)))
        return n.value


class _HashMapBase(_TableCore):
    """the 64-bit-key members: every batch argument is u64[n]"""

    def load_thresholds(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self._L.kh_get_load_thresholds(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_key_transform(self, k):
        """PreTransform of fsc::TransformedHash / TransformedComparator (hash_new.hpp:387-1134): k = 0 identity, k = 1..32
        bliss::kmer::transform::lex_less on 2-bit packed DNA k-mers -- a k-mer and its reverse complement are one key
        ("bimolecule" tables); the bits stored are those of the first occurrence.  Only on an empty table."""
        self._chk(self._L.kh_set_key_transform(self._h, K.KH_XF_DNA_LEX_LESS if k else K.KH_XF_IDENTITY, int(k)))

    # -- batch operations ------------------------------------------------------------------------------
    def insert(self, keys, vals=None):
        """insert(Iter,Iter) / insert(vector const&): first value wins.  Returns #inserted.
        `keys` may also be an (n,2)-shaped uint64 pair array laid out like std::pair<uint64_t,uint32_t>."""
        kb, _, vptr = self._kv(keys, vals)
        new = C.c_uint64()
        if vals is None:
            self._chk(self._L.kh_insert_pairs(self._h, kb.ptr, kb.n // 2, kb.where, C.byref(new)))
        else:
            self._chk(self._L.kh_insert(self._h, kb.ptr, vptr, kb.n, kb.where, C.byref(new)))
        return new.value

    def insert_one(self, key, val):
        """insert(value_type const&): the single-key form -- no trailing reserve(size()) (hashmap_robinhood.hpp:522-626)."""
        out = C.c_uint64()
        self._chk(self._L.kh_insert_one(self._h, int(key), int(val), C.byref(out)))
        return out.value

    def update(self, keys, vals):
        """update(k,v) applied in batch order: insert, or overwrite with the last value given."""
        kb, vb, vptr = self._kv(keys, vals)
        new = C.c_uint64()
        self._chk(self._L.kh_update(self._h, kb.ptr, vptr, kb.n, kb.where, C.byref(new)))
        return new.value

    # -- streamed insert: one insert whose pairs arrive in pieces (multi-GPU exchange) ----------------------------
    def insert_begin(self, n_total, reduce_plus=False, repeatable=False, reduce=None):
        """repeatable: the caller keeps every piece until insert_end has returned and feeds them again (without this flag) if
        insert_end raises KhRetry -- allows the histogram-free partition of the pieces (kh_insert_begin_ex).
        reduce: "plus" | "min" | "max" | "or" -- the streamed form of insert_reduce (reduce_plus=True is reduce="plus")"""
        flags = K.ins_flags(reduce_plus, repeatable, reduce)
        self._chk(self._L.kh_insert_begin_ex(self._h, int(n_total), flags))

    def insert_feed(self, keys, vals=None):
        """partition this piece now (asynchronous for device tensors); the pieces count as one batch in feed order"""
        kb, _, vptr = self._kv(keys, vals)
        self._chk(self._L.kh_insert_feed(self._h, kb.ptr, vptr, kb.n, kb.where))

    def insert_end(self):
        out = C.c_uint64()
        self._chk(self._L.kh_insert_end(self._h, C.byref(out)))
        return out.value

    def insert_abort(self):
        """gives up a streamed insert: the pieces fed so far are dropped, the table is unchanged and usable again"""
        self._chk(self._L.kh_insert_abort(self._h))

    def insert_reduce_plus(self, keys, vals=None):
        """Reducer = std::plus (k-mer counting when vals is None: every occurrence adds 1).  Returns #new keys.
        reference: hashmap_robinhood_offsets_reduction::insert(keys, T(1)), counting_batched_robinhood_map."""
        kb, _, vptr = self._kv(keys, vals)
        new = C.c_uint64()
        self._chk(self._L.kh_insert_reduce_plus(self._h, kb.ptr, vptr, kb.n, kb.where, C.byref(new)))
        return new.value

    def insert_reduce(self, keys, vals=None, op="plus"):
        """reducer insert with Reducer `op`: "plus" (== insert_reduce_plus), "min", "max" (unsigned) or "or" on the 32-bit values.  A new
        key gets the reduction of the values of its occurrences, a key the table holds op(stored, that reduction).  vals may be None
        for "plus" only.  Returns #new keys."""
        rop = K.reduce_op(op)
        if vals is None and rop != K.KH_REDUCE_PLUS:
            raise ValueError("insert_reduce(op=%r) needs values: only 'plus' has a default (1 per occurrence)" % (op,))
        kb, _, vptr = self._kv(keys, vals)
        new = C.c_uint64()
        self._chk(self._L.kh_insert_reduce(self._h, kb.ptr, vptr, kb.n, kb.where, rop, C.byref(new)))
        return new.value

    def count(self, keys, out=None):
        """count(Iter,Iter): 0/1 per query, query order (uint8).  out: a contiguous uint8 CUDA tensor of the queries' length to write
        into (device queries only; nothing is allocated or copied then)."""
        kb = self._query(keys)
        if out is not None and kb.dev:
            assert out.is_contiguous() and out.numel() == kb.n and out.element_size() == 1
            optr = out.data_ptr()
        else:
            out, optr = alloc(kb, kb.n, np.uint8)
        self._chk(self._L.kh_count(self._h, kb.ptr, kb.n, kb.where, optr))
        return out

    def find_values(self, keys, out_vals=None, out_found=None, want_total=True):
        """per-query form: (values, found) aligned with the queries (values of misses are 0).  out_vals / out_found: contiguous
        int32 / uint8 CUDA tensors of the queries' length to write into (device queries only; out_vals must hold 0 where a miss is to
        read 0: the library leaves the values of misses untouched).  want_total=False: the call does not wait for the device."""
        kb = self._query(keys)
        vals, vptr = alloc(kb, kb.n, np.uint32, zero=True) if out_vals is None or not kb.dev else (out_vals, out_vals.data_ptr())
        found, fptr = alloc(kb, kb.n, np.uint8) if out_found is None or not kb.dev else (out_found, out_found.data_ptr())
        if kb.dev:
            assert vals.is_contiguous() and found.is_contiguous() and vals.numel() == kb.n and found.numel() == kb.n
        nf = C.c_uint64()
        self._chk(self._L.kh_find(self._h, kb.ptr, kb.n, kb.where, vptr, fptr, C.byref(nf) if want_total else None))
        return vals, found

    def find(self, keys):
        """find(Iter,Iter): the (key, value) pairs of the hits only, in query order -> (keys, vals)."""
        kb = self._query(keys)
        ok, kptr = alloc(kb, kb.n, np.uint64)
        ov, vptr = alloc(kb, kb.n, np.uint32)
        nf = C.c_uint64()
        self._chk(self._L.kh_find_compact(self._h, kb.ptr, kb.n, kb.where, kptr, vptr, C.byref(nf)))
        return ok[: nf.value], ov[: nf.value]

    def erase(self, keys):
        """erase(Iter,Iter): returns #erased (RH never shrinks here; LP may, as in the reference)."""
        kb = self._query(keys)
        erased = C.c_uint64()
        self._chk(self._L.kh_erase(self._h, kb.ptr, kb.n, kb.where, C.byref(erased)))
        return erased.value

    def erase_one(self, key):
        """erase(key): single-key form, halves the table when size < min_load."""
        out = C.c_uint64()
        self._chk(self._L.kh_erase_one(self._h, int(key), C.byref(out)))
        return out.value

    # -- iteration / exports -----------------------------------------------------------------------------
    def to_vector(self):
        n = self.size()
        k, kptr = alloc(HOST, max(n, 1), np.uint64)
        v, vptr = alloc(HOST, max(n, 1), np.uint32)
        m = C.c_uint64()
        self._chk(self._L.kh_to_vector(self._h, kptr, vptr, C.byref(m)))
        assert m.value == n, (m.value, n)
        return k[:n], v[:n]

    def keys(self):
        return self.to_vector()[0]

    def sorted_items(self):
        k, v = self.to_vector()
        o = np.argsort(k, kind="stable")
        return k[o], v[o]

    def export_slots(self):
        k, kptr = alloc(HOST, self.capacity(), np.uint64)
        v, vptr = alloc(HOST, self.capacity(), np.uint32)
        self._chk(self._L.kh_export_slots(self._h, kptr, vptr))
        return k, v

    # -- measurement ---------------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self._L.kh_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._chk(self._L.kh_profile_reset(self._h))

    def profile(self):
        """{kernel name: (launches, total_ms)} measured with HIP events on the table's stream"""
        return self._profile()


class hashmap_robinhood_doubling(_HashMapBase):
    """fsc::hashmap_robinhood_doubling<uint64_t, uint32_t, Hash> (defaults hashmap_robinhood.hpp:218-220)"""
    KIND = KH_KIND_ROBINHOOD
    DEFAULT_MIN_LF = 0.4
    DEFAULT_MAX_LF = 0.9

    # insert_integrated / insert_sort / insert_shuffled are the same algorithm in the reference
    # (hashmap_robinhood.hpp:721-836,843,1002) minus the trailing reserve(), which is a no-op.
    def insert_integrated(self, keys, vals=None):
        return self.insert(keys, vals)


class hashmap_linearprobe_doubling(_HashMapBase):
    """fsc::hashmap_linearprobe_doubling<uint64_t, uint32_t, Hash> (defaults hashmap_linearprobe.hpp:191-193)"""
    KIND = KH_KIND_LINEARPROBE
    DEFAULT_MIN_LF = 0.2
    DEFAULT_MAX_LF = 0.6


def hash_batch(keys, hash="murmur3avx64", seed=43, device=0, lex_less_k=0):
    """Hash::operator()(Key const*, count, out): batched 64-bit hashing on the GPU; lex_less_k = k: TransformedHash with the
    lex_less pre-transform on 2-bit packed DNA k-mers (hash of min(k-mer, reverse complement))."""
    kb = _Buf.keys(keys)
    hashes, hptr = alloc(kb, kb.n, np.uint64)
    check(K.lib().kh_hash_batch_transformed(_hash_id(hash), seed, K.KH_XF_DNA_LEX_LESS if lex_less_k else K.KH_XF_IDENTITY, int(lex_less_k),
                                            kb.ptr, kb.n, kb.where, hptr, device, stream_of(kb, device)), "kh_hash_batch_transformed")
    return hashes
