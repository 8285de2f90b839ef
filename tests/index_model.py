"""TEST HELPER: numpy model of the k-mer position index (kh_index in include/kmerhash_amd.h).  The reference tree has no multimap of
its own (dsc::multimap is kmerind's), so this model is the yardstick: distinct keys via np.unique, the positions of a key via a stable
sort by (key, pos), window positions derived next to the k-mers of oracle/kmers_np.py (imported, not restated)."""
import numpy as np

from oracle.kmers_np import np_kmers


class IndexModel:
    """key -> ascending positions, from (key, pos) pairs in any order; duplicates kept"""

    def __init__(self, keys, pos):
        keys = np.asarray(keys, dtype=np.uint64)
        pos = np.asarray(pos, dtype=np.uint32)
        assert keys.shape == pos.shape
        order = np.lexsort((pos, keys))                    # stable, by key then position
        self.keys, first, counts = np.unique(keys[order], return_index=True, return_counts=True)
        self.offsets = np.concatenate([first, [len(keys)]]).astype(np.uint64)
        self.positions = pos[order]
        self.counts = counts.astype(np.uint32)

    def size(self):
        return len(self.keys)

    def total(self):
        return len(self.positions)

    def _rank(self, q):
        q = np.asarray(q, dtype=np.uint64)
        r = np.searchsorted(self.keys, q)
        r[r >= len(self.keys)] = 0
        hit = self.keys[r] == q if len(self.keys) else np.zeros(len(q), dtype=bool)
        return r, hit

    def count(self, q):
        r, hit = self._rank(q)
        return np.where(hit, self.counts[r] if len(self.keys) else 0, 0).astype(np.uint32)

    def find(self, q):
        """-> (offsets uint64[len(q) + 1], positions uint32) in query order"""
        c = self.count(q).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)
        r, hit = self._rank(q)
        parts = [self.positions[int(self.offsets[ri]): int(self.offsets[ri + 1])] for ri, h in zip(r, hit) if h]
        pos = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
        return offs, pos

    def export_in_key_order(self, keys_in_slot_order):
        """(offsets uint32, positions uint32) of an export whose keys come in the given (slot) order"""
        r, hit = self._rank(keys_in_slot_order)
        assert hit.all() and len(keys_in_slot_order) == len(self.keys)
        offs = np.concatenate([[0], np.cumsum(self.counts[r].astype(np.uint64))]).astype(np.uint32)
        parts = [self.positions[int(self.offsets[ri]): int(self.offsets[ri + 1])] for ri in r]
        pos = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
        return offs, pos


def np_window_positions(seq, k):
    """byte offsets of the windows np_kmers(seq, k, *) keeps, in its order: the starts of the windows of k valid bases"""
    code = np.full(256, 4, dtype=np.uint8)
    for ch in b"ACGTacgt":
        code[ch] = 0
    c = code[np.asarray(seq, dtype=np.uint8)]
    n = len(c)
    if n < k:
        return np.zeros(0, dtype=np.uint32)
    bad = np.concatenate([[0], np.cumsum(c != 0)])
    ok = (bad[k:] - bad[: n - k + 1]) == 0
    return np.nonzero(ok)[0].astype(np.uint32)


def np_kmers_pos(seq, k, canonical):
    seq = np.asarray(seq, dtype=np.uint8)
    km, pos = np_kmers(seq, k, canonical), np_window_positions(seq, k)
    assert len(km) == len(pos)
    return km, pos


def fastq_masked(text):
    """raw FASTQ text with every byte that is not on a sequence line (line 1 mod 4, the newline that ends a line belonging to it)
    replaced by a newline: same length, so offsets into it are offsets into the raw text"""
    a = np.asarray(text, dtype=np.uint8)
    nl = a == 10
    line = np.concatenate([[0], np.cumsum(nl)[:-1]])
    return np.where(line % 4 == 1, a, 10).astype(np.uint8)


def np_kmers_fastq_pos(text, k, canonical):
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, dtype=np.uint8)
    return np_kmers_pos(fastq_masked(text), k, canonical)


def pack_window(text, p, k, canonical):
    """2-bit packing of text[p:p+k] (A0 C1 G2 T3, first base most significant), canonical: min with the reverse complement"""
    lut = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
    fw = rc = 0
    for j in range(k):
        c = lut[int(text[p + j])]
        fw = (fw << 2) | c
        rc |= (3 - c) << (2 * j)
    return min(fw, rc) if canonical else fw
