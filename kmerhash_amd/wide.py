"""Wide keys: the 16-byte-key Robin Hood table and the 128-bit k-mer front end over the C-ABI (kh_wide_* / kh_kmers128_*).

A wide key is {w0, w1} (two 64-bit words, w0 first in memory).  Batches of keys are numpy uint64 arrays of shape (n, 2) (host memory,
copied by the library) or contiguous torch int64 CUDA tensors of shape (n, 2) (device memory, zero copy); values are (n,) u32.
Results come back in the same kind of container.  A k-mer with k <= 64 is the 128-bit integer V (first base most significant,
A0 C1 G2 T3) stored as w0 = V mod 2^64, w1 = V >> 64."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._capi import KH_KIND_ROBINHOOD, KhError
from .table import _Buf, _TableCore, _hash_id, _is_tensor, torch


def _keys(x):
    """(n, 2) keys -> _Buf over 2n words"""
    if _is_tensor(x) and x.is_cuda:
        if x.dim() != 2 or x.shape[1] != 2:
            raise ValueError("wide keys: expected shape (n, 2), got %s" % (tuple(x.shape),))
        return _Buf(x, np.uint64, 8)
    a = np.asarray(x.cpu().numpy() if _is_tensor(x) else x)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("wide keys: expected shape (n, 2), got %s" % (a.shape,))
    return _Buf(a.astype(np.uint64, copy=False), np.uint64, 8)


class hashmap_robinhood_doubling_wide(_TableCore):
    """fsc::hashmap_robinhood_doubling<Key16, uint32_t, Hash> for 16-byte keys (e.g. Kmer<63, DNA, uint64_t>): the members of
    hashmap_robinhood_doubling for insert / insert_reduce_plus / find / count / erase / reserve / rehash / clear / to_vector.
    Handle and scalar state are _TableCore's over kh_wide_*; none of the 64-bit batch members is inherited."""
    PREFIX = "kh_wide_"
    KIND = KH_KIND_ROBINHOOD
    DEFAULT_MIN_LF = 0.4
    DEFAULT_MAX_LF = 0.9

    def _insert(self, fn, keys, vals):
        kb = _keys(keys)
        vb = _Buf(vals, np.uint32, 4) if vals is not None else None
        if vb is not None and vb.n != kb.n // 2:
            raise ValueError("keys and values differ in length")
        if vb is not None and vb.where != kb.where:
            raise ValueError("keys and values must live in the same memory")
        self._sync_stream(kb, vb)
        out = C.c_uint64()
        self._chk(fn(self._h, kb.ptr, vb.ptr if vb is not None else None, kb.n // 2, kb.where, C.byref(out)))
        return out.value

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
        kb = _keys(keys)
        self._sync_stream(kb)
        n = kb.n // 2
        out, optr = self._out(kb, n, np.uint8, torch.uint8 if torch is not None else None, zero=True)
        self._chk(self._L.kh_wide_count(self._h, kb.ptr, n, kb.where, optr))
        return out

    def find_values(self, keys):
        """per-query form -> (vals, found); vals of misses are 0"""
        kb = _keys(keys)
        self._sync_stream(kb)
        n = kb.n // 2
        vals, vptr = self._out(kb, n, np.uint32, torch.int32 if torch is not None else None, zero=True)
        found, fptr = self._out(kb, n, np.uint8, torch.uint8 if torch is not None else None, zero=True)
        nf = C.c_uint64()
        self._chk(self._L.kh_wide_find(self._h, kb.ptr, n, kb.where, vptr, fptr, C.byref(nf)))
        return vals, found

    def find(self, keys):
        """find(Iter,Iter): the (key, value) pairs of the hits only, in query order -> (keys (m, 2), vals)"""
        kb = _keys(keys)
        self._sync_stream(kb)
        n = kb.n // 2
        ok, kptr = self._out(kb, (n, 2), np.uint64, torch.int64 if torch is not None else None, zero=True)
        ov, vptr = self._out(kb, n, np.uint32, torch.int32 if torch is not None else None, zero=True)
        nf = C.c_uint64()
        self._chk(self._L.kh_wide_find_compact(self._h, kb.ptr, n, kb.where, kptr, vptr, C.byref(nf)))
        return ok[: nf.value], ov[: nf.value]

    def erase(self, keys):
        """erase(Iter,Iter): returns #erased (never shrinks)"""
        kb = _keys(keys)
        self._sync_stream(kb)
        out = C.c_uint64()
        self._chk(self._L.kh_wide_erase(self._h, kb.ptr, kb.n // 2, kb.where, C.byref(out)))
        return out.value

    def to_vector(self):
        n = self.size()
        k = np.zeros((max(n, 1), 2), dtype=np.uint64)
        v = np.zeros(max(n, 1), dtype=np.uint32)
        m = C.c_uint64()
        self._chk(self._L.kh_wide_to_vector(self._h, k.ctypes.data, v.ctypes.data, C.byref(m)))
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
        kb = _keys(keys)
        vb = _Buf(vals, np.uint32, 4) if vals is not None else None
        if vb is not None and (vb.n != kb.n // 2 or vb.where != kb.where):
            raise ValueError("keys/vals must have equal length and live in the same memory space")
        self._sync_stream(kb, vb)
        self._chk(self._L.kh_wide_insert_feed(self._h, kb.ptr, vb.ptr if vb is not None else None, kb.n // 2, kb.where))
        if kb.where == K.KH_MEM_DEVICE:
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
    L = K.lib()
    kb = _keys(keys)
    n = kb.n // 2
    if kb.where == K.KH_MEM_DEVICE:
        out = torch.empty(n, dtype=torch.int64, device=kb.device)
        optr, stream = out.data_ptr(), torch.cuda.current_stream(device).cuda_stream
    else:
        out = np.zeros(n, dtype=np.uint64)
        optr, stream = out.ctypes.data, None
    st = L.kh_wide_hash_batch(_hash_id(hash), seed, kb.ptr, n, kb.where, optr, device, stream)
    if st != K.KH_OK:
        raise KhError(st, "kh_wide_hash_batch")
    return out


def _kmers(fn_name, words, seq, k, canonical, device):
    """shared body of kmers_from_sequence / kmers128_from_sequence (and their FASTQ forms): `words` 64-bit words per k-mer"""
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(seq, dtype=np.uint8)
    b = _Buf(seq, np.uint8, 1)
    shape = max(b.n, 1) if words == 1 else (max(b.n, 1), words)
    n_out = C.c_uint64()
    if b.where == K.KH_MEM_DEVICE:
        out = torch.empty(shape, dtype=torch.int64, device=b.device)
        optr, stream = out.data_ptr(), torch.cuda.current_stream(device).cuda_stream
    else:
        out = np.zeros(shape, dtype=np.uint64)
        optr, stream = out.ctypes.data, None
    st = getattr(K.lib(), fn_name)(b.ptr, b.n, k, 1 if canonical else 0, b.where, optr, C.byref(n_out), device, stream)
    if st != K.KH_OK:
        raise KhError(st, fn_name)
    return out[: n_out.value]


def _kmers_pos(fn_name, seq, k, canonical, device):
    """16-byte k-mers with the byte offsets of their windows (kh_kmers128_from_sequence_pos / _fastq_pos)"""
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(seq, dtype=np.uint8)
    b = _Buf(seq, np.uint8, 1)
    n_out = C.c_uint64()
    if b.where == K.KH_MEM_DEVICE:
        out = torch.empty((max(b.n, 1), 2), dtype=torch.int64, device=b.device)
        pos = torch.empty(max(b.n, 1), dtype=torch.int32, device=b.device)
        optr, pptr, stream = out.data_ptr(), pos.data_ptr(), torch.cuda.current_stream(device).cuda_stream
    else:
        out = np.zeros((max(b.n, 1), 2), dtype=np.uint64)
        pos = np.zeros(max(b.n, 1), dtype=np.uint32)
        optr, pptr, stream = out.ctypes.data, pos.ctypes.data, None
    st = getattr(K.lib(), fn_name)(b.ptr, b.n, k, 1 if canonical else 0, b.where, optr, pptr, C.byref(n_out), device, stream)
    if st != K.KH_OK:
        raise KhError(st, fn_name)
    return out[: n_out.value], pos[: n_out.value]


def kmers128_from_sequence(seq, k=63, canonical=True, device=0, _fastq=False, with_positions=False):
    """-> (n, 2) k-mers (numpy uint64 for host input, torch int64 CUDA tensor for device input), sequence order; k = 1..64.
    with_positions: -> (k-mers, positions): positions[i] (numpy uint32 / torch int32) is the byte offset in `seq` of the first base of
    the window that gave k-mers[i] (a text of 2^32 bytes or more is refused)"""
    if with_positions:
        return _kmers_pos("kh_kmers128_from_fastq_pos" if _fastq else "kh_kmers128_from_sequence_pos", seq, k, canonical, device)
    return _kmers("kh_kmers128_from_fastq" if _fastq else "kh_kmers128_from_sequence", 2, seq, k, canonical, device)


def kmers128_from_fastq(text, k=63, canonical=True, device=0, with_positions=False):
    """raw FASTQ text (whole 4-line records) -> (n, 2) k-mers of the sequence lines (record structure resolved on the GPU);
    with_positions: -> (k-mers, byte offsets of their windows in the raw text)"""
    return kmers128_from_sequence(text, k, canonical, device, _fastq=True, with_positions=with_positions)


def syncmers128_from_sequence(seq, k=63, s=31, canonical=True, order_hash="murmur", order_seed=42, device=0, _fastq=False):
    """closed syncmers of `seq` as 16-byte k-mers, k = 1..64, s = 1..min(k, 32) -> ((m, 2) k-mers, positions), ascending positions: the
    windows of kmers128_from_sequence(with_positions=True) whose smallest s-mer by order_hash (of the canonical s-mer when `canonical`)
    is the first or the last of the k - s + 1 (kh_syncmers128_from_sequence; kmerhash_amd.syncmers_from_sequence for the definition)"""
    from .kmers import _syncmers
    return _syncmers("kh_syncmers128_from_fastq" if _fastq else "kh_syncmers128_from_sequence", 2, seq, k, s, canonical, order_hash, order_seed, device)


def syncmers128_from_fastq(text, k=63, s=31, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """syncmers128_from_sequence over the sequence lines of raw FASTQ text (whole 4-line records); positions are byte offsets into the text"""
    return syncmers128_from_sequence(text, k, s, canonical, order_hash, order_seed, device, _fastq=True)


def is_syncmer128(keys, k=63, s=31, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """for (n, 2) 16-byte k-mers: a bool array / tensor, True where the k-mer is a closed syncmer under these parameters (kh_wide_syncmer_mask)"""
    from .kmers import _syncmer_mask
    kb = _keys(keys)
    return _syncmer_mask("kh_wide_syncmer_mask", kb, kb.n // 2, k, s, canonical, order_hash, order_seed, device)
