"""TEST HELPER (not collected): the model behind the random operation sequences over the two position indexes (kh_index_* and
kh_wide_index_* in include/kmerhash_amd.h).  PairBag is an index as the multiset of (key, position) pairs given so far -- numpy only, no
hash table --, as_model() turns it into what a per-call check compares with (an IndexModel for 8-byte keys, the same interface for
16-byte keys, both with vectorised find / export), and text_pairs() states which pairs a text call must add: the windows of
tests/index_model.py and tests/syncmer_model.py, the stamp of tests/strand_model.py and the selections of tests/minimizer_model.py and
tests/syncmer_model.py, all imported.  A key is a row of `words` uint64: (w0,) or (w0, w1), ordered by w1 first."""
import functools

import numpy as np

from tests.index_model import IndexModel, fastq_masked, np_kmers_fastq_pos, np_kmers_pos, np_window_positions
from tests.minimizer_model import np_minimizers, np_minimizers_fastq
from tests.strand_model import np_stamp
from tests.syncmer_model import np_kmers128, np_syncmers, np_syncmers_fastq

ORDER_HASH, ORDER_SEED = "murmur", 42          # the sampler defaults of KmerPositionIndex.__init__
U32 = 1 << 32


# ---- rows of 8- or 16-byte keys: the one place that sorts and ranks them ------------------------------------------------------------
def key_rows(keys, words):
    """any key batch as a C-contiguous (n, words) uint64 array"""
    return np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1, words))


def row_order(rows, *minor):
    """argsort of rows by (last word, ..., first word), ties by the minor keys given (the first one given varies fastest)"""
    return np.lexsort(tuple(minor) + tuple(rows[:, j] for j in range(rows.shape[1])))


def unique_rows(rows):
    """-> (distinct rows ascending, counts int64)"""
    if len(rows) == 0:
        return rows[:0].copy(), np.zeros(0, dtype=np.int64)
    s = rows[row_order(rows)]
    new = np.ones(len(s), dtype=bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    first = np.nonzero(new)[0]
    return s[first], np.diff(np.concatenate([first, [len(s)]])).astype(np.int64)


def rank_rows(u, q):
    """u: distinct rows ascending.  -> (rank int64[len(q)], hit bool[len(q)]): u[rank[i]] == q[i] where hit[i] (rank 0 otherwise)"""
    nu, nq = len(u), len(q)
    if nu == 0 or nq == 0:
        return np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=bool)
    both = np.concatenate([u, q])
    order = row_order(both, np.arange(nu + nq) >= nu)              # among equal rows the one of u stands first
    last = np.maximum.accumulate(np.where(order < nu, order, -1))  # (a row of u has its rank as its index)
    r = np.empty(nu + nq, dtype=np.int64)
    r[order] = last
    r = np.maximum(r[nu:], 0)
    hit = (u[r] == q).all(axis=1)
    return np.where(hit, r, 0), hit


def isin_rows(rows, other):
    return rank_rows(unique_rows(other)[0], rows)[1]


# ---- the per-call yardstick -----------------------------------------------------------------------------------------------------------
class _Gather:
    """find and export_in_key_order without a Python loop over keys or queries: needs keys (ascending), offsets, counts, positions"""
    WORDS = 1

    def _rank(self, q):
        return rank_rows(key_rows(self.keys, self.WORDS), key_rows(q, self.WORDS))

    def _segments(self, r, hit):
        c = np.where(hit, self.counts[r] if len(self.counts) else 0, 0).astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        start = (self.offsets[r].astype(np.int64) if len(self.counts) else np.zeros(len(r), dtype=np.int64)) - offs[:-1]
        idx = np.repeat(start, c) + np.arange(offs[-1])
        return offs, self.positions[idx].astype(np.uint32)

    def size(self):
        return len(self.keys)

    def total(self):
        return len(self.positions)

    def count(self, q):
        r, hit = self._rank(q)
        return np.where(hit, self.counts[r] if len(self.counts) else 0, 0).astype(np.uint32)

    def find(self, q):
        """-> (offsets uint64[len(q) + 1], positions uint32) in query order"""
        offs, pos = self._segments(*self._rank(q))
        return offs.astype(np.uint64), pos

    def export_in_key_order(self, keys_in_slot_order):
        """(offsets uint32, positions uint32) of an export whose keys come in the given (slot) order: every key once"""
        r, hit = self._rank(keys_in_slot_order)
        assert hit.all() and len(r) == len(self.keys) and len(np.unique(r)) == len(r)
        offs, pos = self._segments(r, hit)
        return offs.astype(np.uint32), pos


class NarrowSeqModel(_Gather, IndexModel):
    """IndexModel (its constructor, its fields) with the vectorised lookups"""


class WideSeqModel(_Gather):
    """the same over (w0, w1) rows, ascending by (w1, w0)"""
    WORDS = 2

    def __init__(self, keys, pos):
        keys, pos = key_rows(keys, 2), np.asarray(pos, dtype=np.uint32)
        assert len(keys) == len(pos)
        order = row_order(keys, pos)
        self.keys, counts = unique_rows(keys)
        self.offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        self.positions = pos[order]
        self.counts = counts.astype(np.uint32)


# ---- the index as a bag of pairs ------------------------------------------------------------------------------------------------------
class PairBag:
    """the multiset of (key, pos) pairs an index holds; duplicates kept"""

    def __init__(self, words):
        self.words = int(words)
        self.clear()

    def clear(self):
        self.keys, self.pos = np.zeros((0, self.words), dtype=np.uint64), np.zeros(0, dtype=np.uint32)

    def append(self, keys, pos):
        keys, pos = key_rows(keys, self.words), np.asarray(pos, dtype=np.uint32).ravel()
        assert len(keys) == len(pos)
        self.keys, self.pos = np.concatenate([self.keys, keys]), np.concatenate([self.pos, pos])
        return len(pos)

    def size(self):
        return len(unique_rows(self.keys)[0])

    def total(self):
        return len(self.pos)

    def live(self):
        """-> (distinct keys ascending, their counts)"""
        return unique_rows(self.keys)

    def erase(self, keys):
        """-> (distinct keys erased, positions erased); misses and repeats in the batch are harmless"""
        gone = isin_rows(self.keys, key_rows(keys, self.words))
        nk, npos = len(unique_rows(self.keys[gone])[0]), int(gone.sum())
        self.keys, self.pos = self.keys[~gone], self.pos[~gone]
        return nk, npos

    def erase_counts(self, lo, hi):
        """every key whose count lies in [lo, hi] (lo > hi: the empty range) -> (keys, positions)"""
        u, c = self.live()
        return self.erase(u[(c >= int(lo)) & (c <= int(hi))])

    def drop_above(self, max_occ):
        return (0, 0) if int(max_occ) >= U32 - 1 else self.erase_counts(int(max_occ) + 1, U32 - 1)

    def as_model(self):
        return NarrowSeqModel(self.keys[:, 0], self.pos) if self.words == 1 else WideSeqModel(self.keys, self.pos)


# ---- what a text call adds -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=256)
def _text_pairs(raw, k, canonical, fastq, pos_base, stranded, w, s, wide):
    text = np.frombuffer(raw, dtype=np.uint8)
    if w is not None:
        assert not wide and s is None
        km, pos = (np_minimizers_fastq if fastq else np_minimizers)(text, k, w, canonical, ORDER_HASH, ORDER_SEED)
    elif s is not None:
        km, pos = (np_syncmers_fastq if fastq else np_syncmers)(text, k, s, canonical, ORDER_HASH, ORDER_SEED, wide)
    elif wide:
        masked = fastq_masked(text) if fastq else text
        km, pos = np_kmers128(masked, k, canonical), np_window_positions(masked, k)
    else:
        km, pos = (np_kmers_fastq_pos if fastq else np_kmers_pos)(text, k, canonical)
    assert len(km) == len(pos)
    if stranded:
        # (on the raw text: a window of a FASTQ sequence line is k bases there too)
        assert int(pos_base) + len(text) <= 1 << 31
        stored = np_stamp(text, pos, k, pos_base)
        assert (stored != 0xFFFFFFFF).all()                    # (every window the model emits is a valid one)
    else:
        assert int(pos_base) + len(text) <= U32
        stored = (pos.astype(np.int64) + int(pos_base)).astype(np.uint32)
    km = key_rows(km, 2 if wide else 1)
    km.setflags(write=False)
    stored.setflags(write=False)
    return km, stored


def text_pairs(text, k, canonical=True, fastq=False, pos_base=0, stranded=False, w=None, s=None, wide=False):
    """the pairs a text call puts into the index -> (keys (n, words) uint64, stored positions uint32) in text order; stored = pos_base
    + window offset, or the stamp ((pos_base + p) << 1) | rc(p) on a stranded index.  Read-only arrays, cached per argument tuple."""
    raw = bytes(text) if isinstance(text, (bytes, bytearray)) else np.asarray(text, dtype=np.uint8).tobytes()
    return _text_pairs(raw, int(k), bool(canonical), bool(fastq), int(pos_base), bool(stranded), w, s, bool(wide))
