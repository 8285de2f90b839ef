"""Wide keys: the 16-byte-key Robin Hood table and the 128-bit k-mer front end over the C-ABI (kh_wide_* / kh_kmers128_*).

A wide key is {w0, w1} (two 64-bit words, w0 first in memory).  Batches of keys are numpy uint64 arrays of shape (n, 2) (host memory,
copied by the library) or contiguous torch int64 CUDA tensors of shape (n, 2) (device memory, zero copy); values are (n,) u32.
Results come back in the same kind of container.  A k-mer with k <= 64 is the 128-bit integer V (first base most significant,
A0 C1 G2 T3) stored as w0 = V mod 2^64, w1 = V >> 64."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._call import HOST, _Buf, alloc, check, stream_of
from ._capi import KH_KIND_ROBINHOOD
from .seqs import (is_syncmer128, kmers128_from_fastq, kmers128_from_sequence, syncmers128_from_fastq,  # noqa: F401  (re-exported)
                   syncmers128_from_sequence)
from .table import _TableCore, _hash_id


class hashmap_robinhood_doubling_wide(_TableCore):
    """fsc::hashmap_robinhood_doubling<Key16, uint32_t, Hash> for 16-byte keys (e.g. Kmer<63, DNA, uint64_t>): the members of
    hashmap_robinhood_doubling for insert / insert_reduce_plus / find / count / erase / reserve / rehash / clear / to_vector.
    Handle and scalar state are _TableCore's over kh_wide_*; none of the 64-bit batch members is inherited."""
    PREFIX = "kh_wide_"
    WORDS = 2
    KIND = KH_KIND_ROBINHOOD
    DEFAULT_MIN_LF = 0.4
    DEFAULT_MAX_LF = 0.9

    def _insert(self, fn, keys, vals):
        kb, _, vptr = self._kv(keys, vals, "keys and values differ in length", "keys and values must live in the same memory")
        new = C.c_uint64()
        self._chk(fn(self._h, kb.ptr, vptr, kb.n, kb.where, C.byref(new)))
        return new.value

    def insert(self, keys, vals):
        """insert(Iter,Iter): first value wins; returns the number of new keys"""
        return self._insert(self._L.kh_wide_insert, keys, vals)

    def insert_reduce_plus(self, keys, vals=None):
        """Reducer = std::plus (wrapping 32-bit); vals None: every occurrence counts 1"""
        return self._insert(self._L.kh_wide_insert_reduce_plus, keys, vals)

    def insert_reduce(self, keys, vals=None, op="plus"):
        """reducer insert with Reducer `op`: "plus" (== insert_reduce_plus), "min", "max" (unsigned) or "or"; vals may be None for
        "plus" only"""
        rop = K.reduce_op(op)
        if vals is None and rop != K.KH_REDUCE_PLUS:
            raise ValueError("insert_reduce(op=%r) needs values: only 'plus' has a default (1 per occurrence)" % (op,))
        return self._insert(lambda h, k, v, n, where, out: self._L.kh_wide_insert_reduce(h, k, v, n, where, rop, out), keys, vals)

    def count(self, keys):
        kb = self._query(keys)
        out, optr = alloc(kb, kb.n, np.uint8, zero=True)
        self._chk(self._L.kh_wide_count(self._h, kb.ptr, kb.n, kb.where, optr))
        return out

    def find_values(self, keys):
        """per-query form -> (vals, found); vals of misses are 0"""
        kb = self._query(keys)
        vals, vptr = alloc(kb, kb.n, np.uint32, zero=True)
        found, fptr = alloc(kb, kb.n, np.uint8, zero=True)
        nf = C.c_uint64()
        self._chk(self._L.kh_wide_find(self._h, kb.ptr, kb.n, kb.where, vptr, fptr, C.byref(nf)))
        return vals, found

    def find(self, keys):
        """find(Iter,Iter): the (key, value) pairs of the hits only, in query order -> (keys (m, 2), vals)"""
        kb = self._query(keys)
        ok, kptr = alloc(kb, (kb.n, 2), np.uint64, zero=True)
        ov, vptr = alloc(kb, kb.n, np.uint32, zero=True)
        nf = C.c_uint64()
        self._chk(self._L.kh_wide_find_compact(self._h, kb.ptr, kb.n, kb.where, kptr, vptr, C.byref(nf)))
        return ok[: nf.value], ov[: nf.value]

    def erase(self, keys):
        """erase(Iter,Iter): returns #erased (never shrinks)"""
        kb = self._query(keys)
        erased = C.c_uint64()
        self._chk(self._L.kh_wide_erase(self._h, kb.ptr, kb.n, kb.where, C.byref(erased)))
        return erased.value

    def to_vector(self):
        n = self.size()
        k, kptr = alloc(HOST, (max(n, 1), 2), np.uint64)
        v, vptr = alloc(HOST, max(n, 1), np.uint32)
        m = C.c_uint64()
        self._chk(self._L.kh_wide_to_vector(self._h, kptr, vptr, C.byref(m)))
        assert m.value == n, (m.value, n)
        return k[:n], v[:n]

    def keys(self):
        return self.to_vector()[0]

    def sorted_items(self):
        """to_vector() sorted by (w1, w0)"""
        k, v = self.to_vector()
        o = np.lexsort((k[:, 0], k[:, 1]))
        return k[o], v[o]


class hashmap_robinhood_doubling_wide_stream(hashmap_robinhood_doubling_wide):
    """hashmap_robinhood_doubling_wide plus the streamed insert (kh_wide_insert_begin_ex / feed / end / abort): ONE insert whose
    (n, 2) key pieces arrive one by one -- what the multi-GPU layer feeds as its exchanges land.  The result equals insert() /
    insert_reduce_plus() of the pieces concatenated in feed order.  Device pieces must stay alive and unchanged until insert_end()
    or insert_abort() has returned (the object keeps a reference to each)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._fed = []          # device pieces of the streamed insert in progress

    def insert_begin(self, n_total, reduce_plus=False, repeatable=False, reduce=None):
        """repeatable is accepted for the interface of the 64-bit table; a wide table never raises KhRetry.
        reduce: "plus" | "min" | "max" | "or" -- the streamed form of insert_reduce (reduce_plus=True is reduce="plus")"""
        flags = K.ins_flags(reduce_plus, repeatable, reduce)
        self._chk(self._L.kh_wide_insert_begin_ex(self._h, int(n_total), flags))
        self._fed = []

    def insert_feed(self, keys, vals=None):
        """count this piece's partitions now (asynchronous for device tensors); the pieces count as one batch in feed order"""
        kb, vb, vptr = self._kv(keys, vals)
        self._chk(self._L.kh_wide_insert_feed(self._h, kb.ptr, vptr, kb.n, kb.where))
        if kb.dev:
            self._fed.append((kb.obj, vb.obj if vb is not None else None))

    def insert_end(self):
        out = C.c_uint64()
        try:
            self._chk(self._L.kh_wide_insert_end(self._h, C.byref(out)))
        finally:
            self._fed = []
        return out.value

    def insert_abort(self):
        """gives up a streamed insert: the pieces fed so far are dropped, the table is unchanged and usable again"""
        try:
            self._chk(self._L.kh_wide_insert_abort(self._h))
        finally:
            self._fed = []


def hash_batch_wide(keys, hash="murmur3avx64", seed=43, device=0):
    """Hash::operator()(Key const*, count, out) for 16-byte keys: (n, 2) keys -> n 64-bit hashes"""
    kb = _Buf.keys(keys, 2)
    hashes, hptr = alloc(kb, kb.n, np.uint64)
    check(K.lib().kh_wide_hash_batch(_hash_id(hash), seed, kb.ptr, kb.n, kb.where, hptr, device, stream_of(kb, device)), "kh_wide_hash_batch")
    return hashes
