"""TEST HELPER (not collected): numpy / Python-integer model of the strand bit and the stamped position (kh_stamp_strand in
include/kmerhash_amd.h).  It states the definition directly, one window at a time on Python integers: a window of k bases is packed
first base most significant (A0 C1 G2 T3), its reverse complement likewise, and rc = 1 iff the reverse complement is STRICTLY smaller.
A window that passes the end of the text or holds a byte that is no base is invalid."""
import numpy as np

POS_INVALID = 0xFFFFFFFF
LUT = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def revcomp_text(text):
    """reverse complement of a text of bases (case kept)"""
    return COMP[np.asarray(text, dtype=np.uint8)[::-1]].copy()


def strand_bit(text, p, k):
    """rc(p) of the window text[p:p + k] from the definition, or None for an invalid window"""
    n = len(text)
    if p < 0 or p + k > n:
        return None
    fw = rc = 0
    for j in range(k):
        c = LUT.get(int(text[p + j]))
        if c is None:
            return None
        fw = (fw << 2) | c
        rc |= (3 - c) << (2 * j)
    return 1 if rc < fw else 0


def np_strand_bits(text, pos, k):
    """-> (bits uint8[m], valid bool[m]) for the windows at `pos` (any order, repeats allowed; invalid windows have bit 0)"""
    text = np.asarray(text, dtype=np.uint8)
    pos = np.asarray(pos, dtype=np.int64)
    bits, valid = np.zeros(len(pos), dtype=np.uint8), np.zeros(len(pos), dtype=bool)
    memo = {}
    for i, p in enumerate(pos):
        p = int(p)
        if p not in memo:
            memo[p] = strand_bit(text, p, k)
        if memo[p] is not None:
            bits[i], valid[i] = memo[p], True
    return bits, valid


def np_stamp(text, pos, k, pos_base=0):
    """-> uint32[m]: ((pos_base + p) << 1) | rc(p), POS_INVALID for an invalid window"""
    bits, valid = np_strand_bits(text, pos, k)
    v = ((np.asarray(pos, dtype=np.int64) + int(pos_base)) << 1) | bits
    return np.where(valid, v, POS_INVALID).astype(np.uint32)
