"""TEST HELPER: numpy model of the position index over 16-byte keys (kh_wide_index_* in include/kmerhash_amd.h).  A key is a row
(w0, w1) of a uint64 array and stands for the 128-bit value (w1 << 64) | w0; distinct keys come in ascending order of that value, the
positions of a key ascend (np.lexsort((pos, w0, w1)): w1 is the major key).  Window positions and the packing of a window are those of
tests/index_model.py, which work for any k on Python integers."""
import numpy as np

from index_model import np_window_positions, pack_window  # noqa: F401  (re-exported for the tests)

M64 = (1 << 64) - 1


def split128(v):
    """128-bit Python integer -> (w0, w1)"""
    return v & M64, v >> 64


def pack_window128(text, p, k, canonical):
    """(w0, w1) of the k-mer of text[p:p+k], k = 1..64"""
    return split128(pack_window(text, p, k, canonical))


def kmers128_pos_model(text, k, canonical):
    """-> (k-mers uint64 (n, 2), positions uint32): every window of k valid bases in text order"""
    pos = np_window_positions(text, k)
    km = np.array([pack_window128(text, int(p), k, canonical) for p in pos], dtype=np.uint64).reshape(-1, 2)
    return km, pos


class WideIndexModel:
    """(w0, w1) key -> ascending positions, from (key, pos) pairs in any order; duplicates kept"""

    def __init__(self, keys, pos):
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 2)
        pos = np.asarray(pos, dtype=np.uint32)
        assert len(keys) == len(pos)
        n = len(pos)
        order = np.lexsort((pos, keys[:, 0], keys[:, 1]))           # by w1, then w0, then position
        sk = keys[order]
        new = np.ones(n, dtype=bool)
        new[1:] = (sk[1:] != sk[:-1]).any(axis=1)
        first = np.nonzero(new)[0]
        self.keys = sk[first]
        self.offsets = np.concatenate([first, [n]]).astype(np.uint64)
        self.positions = pos[order]
        self.counts = np.diff(self.offsets.astype(np.int64)).astype(np.uint32)
        self._rank_of = {(int(a), int(b)): r for r, (a, b) in enumerate(self.keys)}

    def size(self):
        return len(self.keys)

    def total(self):
        return len(self.positions)

    def _rank(self, q):
        q = np.asarray(q, dtype=np.uint64).reshape(-1, 2)
        return [self._rank_of.get((int(a), int(b)), -1) for a, b in q]

    def count(self, q):
        return np.array([self.counts[r] if r >= 0 else 0 for r in self._rank(q)], dtype=np.uint32)

    def find(self, q):
        """-> (offsets uint64[len(q) + 1], positions uint32) in query order"""
        ranks = self._rank(q)
        c = np.array([self.counts[r] if r >= 0 else 0 for r in ranks], dtype=np.uint64)
        offs = np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)
        parts = [self.positions[int(self.offsets[r]): int(self.offsets[r + 1])] for r in ranks if r >= 0]
        pos = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
        return offs, pos

    def export_in_key_order(self, keys_in_slot_order):
        """(offsets uint32, positions uint32) of an export whose keys come in the given (slot) order"""
        ranks = self._rank(keys_in_slot_order)
        assert all(r >= 0 for r in ranks) and len(ranks) == len(self.keys) and len(set(ranks)) == len(ranks)
        offs = np.concatenate([[0], np.cumsum(self.counts[ranks].astype(np.uint64))]).astype(np.uint32) if ranks else np.zeros(1, dtype=np.uint32)
        parts = [self.positions[int(self.offsets[r]): int(self.offsets[r + 1])] for r in ranks]
        pos = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
        return offs, pos
