"""CPU model of the 16-byte-key Robin Hood table (hashmap_robinhood_doubling_wide).  TEST INFRASTRUCTURE ONLY; no GPU, no torch.

The model is composed of three independent parts, none of which is code of the table under test:

  scalar rules   size, capacity, return values and the one-doubling-per-call rule come from the 64-bit CPU oracle
                 (OracleTable(KIND_RH)), fed SURROGATE keys: the index of each distinct 16-byte key in first-seen order, plus 1.
                 The capacity rule depends only on counts and on where in the batch the last new key first occurs; an injective
                 map of the keys preserves both.  The surrogate table hashes with murmur3, so it never overflows a probe itself.
  values         a Python dict: first value wins (insert) or sums wrap mod 2^32 (insert_reduce_plus).
  layout         the canonical Robin Hood info array over the homes at the current capacity (rh_info_model: elements sorted by
                 home, slot = max(home, previous slot + 1), circular).  The homes come from the oracle's own hashes of the 16 key
                 bytes (ora_hash16_batch), never from the GPU library.

A call whose resulting layout would need a probe distance of 128 or more is refused: the model sets `probe_overflow`, returns None
and stays as it was before the call -- what the table does with KH_ERR_PROBE_OVERFLOW."""
import numpy as np

from . import oracle_py as O

M32 = 0xFFFFFFFF
HASH_IDS = {"identity": O.HASH_IDENTITY, "murmur3avx64": O.HASH_MURMUR3_X86, "murmur": O.HASH_MURMUR3_X64, "farm": O.HASH_FARM}


def rh_positions(h, cap):
    """h: homes in ascending order -> unwrapped slot of each element (slot = position % cap): slot = max(home, previous slot + 1),
    circular ((max,+) scan run twice around the circle)"""
    idx = np.arange(len(h), dtype=np.int64)
    p = idx + np.maximum.accumulate(h - idx)
    x0 = max(0, int(p[-1]) + 1 - cap)                 # run-over of the last home into the start of the table
    return idx + np.maximum(np.maximum.accumulate(h - idx), x0)


def rh_max_distance(homes, cap):
    """largest probe distance of the canonical layout (-1: no elements)"""
    h = np.sort(np.asarray(homes, dtype=np.int64))
    return int((rh_positions(h, cap) - h).max()) if len(h) else -1


def rh_info_model(homes, cap):
    """canonical Robin Hood info array: elements sorted by home, slot = max(home, previous slot + 1), circular ((max,+) scan run twice
    around the circle)"""
    h = np.sort(np.asarray(homes, dtype=np.int64))
    info = np.zeros(cap, dtype=np.uint8)
    if len(h) == 0:
        return info
    p = rh_positions(h, cap)
    dist = p - h
    assert dist.max() < 128
    info[p % cap] = 0x80 | dist
    return info


def as_keys(keys):
    a = np.ascontiguousarray(keys, dtype=np.uint64)
    return a.reshape(-1, 2)


class WideModel:
    def __init__(self, capacity=128, min_lf=0.4, max_lf=0.9, hash="murmur3avx64", seed=43):
        self.hash_id = HASH_IDS[hash] if isinstance(hash, str) else int(hash)
        self.seed = seed
        self.min_lf, self.max_lf = min_lf, max_lf
        self._o = O.OracleTable(O.KIND_RH, capacity, min_lf, max_lf, O.HASH_MURMUR3_X86, 43)
        self._sur = {}            # (w0, w1) -> surrogate 64-bit key; never forgotten
        self._d = {}              # live (w0, w1) -> value
        self.probe_overflow = False       # set by the last mutating call if it was refused

    # ---- parts ------------------------------------------------------------------------------------
    def _surrogates(self, kt):
        s = self._sur
        out = np.empty(len(kt), dtype=np.uint64)
        for i, k in enumerate(kt):
            v = s.get(k)
            if v is None:
                v = s[k] = len(s) + 1
            out[i] = v
        return out

    def hashes(self, keys):
        return O.hash16_batch(self.hash_id, self.seed, as_keys(keys))

    def homes(self, keys):
        """home slot of each key at the current capacity"""
        return self.hashes(keys) & np.uint64(self.capacity() - 1)

    def _live_keys(self):
        return np.array(list(self._d.keys()), dtype=np.uint64).reshape(-1, 2)

    def _commit(self, snap, ret):
        """the call has been applied to the three parts: keep it if the layout exists, else put everything back"""
        self.probe_overflow = False
        assert self._o.size() == len(self._d), (self._o.size(), len(self._d))
        if self._d:
            if rh_max_distance(self.homes(self._live_keys()).astype(np.int64), self.capacity()) >= 128:
                d, cap = snap
                self._d = d
                # the surrogate table again at the old size and capacity: filled under a max load factor no insert reaches
                self._o = O.OracleTable(O.KIND_RH, cap, self.min_lf, 4.0, O.HASH_MURMUR3_X86, 43)
                sur = self._surrogates(list(d.keys()))
                self._o.insert(sur, np.zeros(len(sur), dtype=np.uint32))
                self._o.set_max_load_factor(self.max_lf)
                assert (self._o.size(), self._o.capacity()) == (len(d), cap)
                self.probe_overflow = True
                return None
        return ret

    def _snap(self):
        return dict(self._d), self._o.capacity()

    # ---- the members of hashmap_robinhood_doubling_wide ---------------------------------------------
    def size(self):
        return self._o.size()

    def capacity(self):
        return self._o.capacity()

    def set_min_load_factor(self, f):
        self.min_lf = f
        self._o.set_min_load_factor(f)

    def set_max_load_factor(self, f):
        self.max_lf = f
        self._o.set_max_load_factor(f)

    def insert(self, keys, vals):
        """first value wins; -> number of new keys (None: refused, probe overflow)"""
        kt = list(map(tuple, as_keys(keys).tolist()))
        vals = np.asarray(vals, dtype=np.uint32).tolist()
        assert len(vals) == len(kt)
        snap = self._snap()
        sur = self._surrogates(kt)
        r = self._o.insert(sur, np.zeros(len(sur), dtype=np.uint32))
        d = self._d
        for k, v in zip(kt, vals):
            d.setdefault(k, v)
        return self._commit(snap, r)

    def insert_reduce_plus(self, keys, vals=None):
        """Reducer = std::plus, wrapping 32-bit; vals None: every occurrence counts 1.  Membership, size and capacity: ONE insert of
        the batch on the surrogate table (the construction of oracle_plus in tests/soak_fuzz.py)"""
        kt = list(map(tuple, as_keys(keys).tolist()))
        vals = [1] * len(kt) if vals is None else np.asarray(vals, dtype=np.uint32).tolist()
        assert len(vals) == len(kt)
        snap = self._snap()
        sur = self._surrogates(kt)
        r = self._o.insert(sur, np.zeros(len(sur), dtype=np.uint32))
        d = self._d
        for k, v in zip(kt, vals):
            d[k] = (d.get(k, 0) + v) & M32
        return self._commit(snap, r)

    def erase(self, keys):
        kt = list(map(tuple, as_keys(keys).tolist()))
        snap = self._snap()
        r = self._o.erase(self._surrogates(kt))
        for k in kt:
            self._d.pop(k, None)
        return self._commit(snap, r)

    def reserve(self, n):
        snap = self._snap()
        self._o.reserve(int(n))
        return self._commit(snap, None)

    def rehash(self, b):
        """raises RuntimeError where the oracle's rehash throws"""
        snap = self._snap()
        self._o.rehash(int(b))
        return self._commit(snap, None)

    def clear(self):
        self._o.clear()
        self._d.clear()
        self.probe_overflow = False

    def count(self, keys):
        d = self._d
        return np.array([1 if k in d else 0 for k in map(tuple, as_keys(keys).tolist())], dtype=np.uint8)

    def find_values(self, keys):
        """per-query form -> (vals, found); vals of misses are 0"""
        d = self._d
        kt = list(map(tuple, as_keys(keys).tolist()))
        found = np.array([1 if k in d else 0 for k in kt], dtype=np.uint8)
        vals = np.array([d.get(k, 0) for k in kt], dtype=np.uint32)
        return vals, found

    def find(self, keys):
        """the (key, value) pairs of the hits only, in query order -> (keys (m, 2), vals)"""
        d = self._d
        hits = [k for k in map(tuple, as_keys(keys).tolist()) if k in d]
        return np.array(hits, dtype=np.uint64).reshape(-1, 2), np.array([d[k] for k in hits], dtype=np.uint32)

    def export_info(self):
        return rh_info_model(self.homes(self._live_keys()).astype(np.int64), self.capacity())

    def displacement_histogram(self):
        info = self.export_info()
        return np.bincount(info[info >= 0x80] & 0x7F, minlength=128).astype(np.uint64)

    def sorted_items(self):
        """(keys, vals) sorted by (w1, w0)"""
        k = self._live_keys()
        v = np.array(list(self._d.values()), dtype=np.uint32)
        o = np.lexsort((k[:, 0], k[:, 1]))
        return k[o], v[o]

    def close(self):
        self._o.close()
