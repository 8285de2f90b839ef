"""TEST HELPER: numpy model of closed-syncmer sampling (kh_syncmers_from_sequence / kh_syncmers128_from_sequence / kh_syncmer_mask in
include/kmerhash_amd.h).  The reference tree has no sampler, so this model is the yardstick.  It states the definition directly: valid
windows and 8-byte k-mers from oracle/kmers_np.py and tests/index_model.py (imported, not restated), the order keys of the s-mers from
the CPU hash oracle.oracle_py.hash_batch -- never the GPU library's hash --, and per valid window the minimum over its k - s + 1 keys
compared with the first and the last of them.  16-byte k-mers ({w0, w1} rows) are packed here, word by word, since the oracle's packer
stops at k = 32."""
import numpy as np

from oracle.kmers_np import np_kmers
from tests.index_model import fastq_masked, np_window_positions
from tests.minimizer_model import order_keys

M64 = (1 << 64) - 1


def _codes(seq):
    code = np.full(256, 4, dtype=np.uint8)
    for ch, c in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        code[ch] = c
    return code[np.asarray(seq, dtype=np.uint8)]


def np_kmers128(seq, k, canonical):
    """every window of k valid bases as a row (w0, w1) of the 128-bit k-mer (first base most significant), k = 1..64, in text order"""
    c = _codes(seq)
    n = len(c)
    if n < k:
        return np.zeros((0, 2), dtype=np.uint64)
    pos = np_window_positions(seq, k).astype(np.int64)
    cc = (c & 3).astype(np.uint64)
    m = n - k + 1
    two, sixty2 = np.uint64(2), np.uint64(62)
    fhi = np.zeros(m, dtype=np.uint64); flo = np.zeros(m, dtype=np.uint64)
    rhi = np.zeros(m, dtype=np.uint64); rlo = np.zeros(m, dtype=np.uint64)
    for j in range(k):
        b = cc[j: m + j]
        fhi = (fhi << two) | (flo >> sixty2)
        flo = (flo << two) | b
        comp = np.uint64(3) - b
        if j < 32:
            rlo |= comp << np.uint64(2 * j)
        else:
            rhi |= comp << np.uint64(2 * (j - 32))
    if canonical:
        take_rc = (rhi < fhi) | ((rhi == fhi) & (rlo < flo))
        flo = np.where(take_rc, rlo, flo); fhi = np.where(take_rc, rhi, fhi)
    return np.stack([flo[pos], fhi[pos]], axis=1)


def smer_keys(seq, s, canonical, hash_id, seed):
    """-> (keys uint64[n], valid bool[n]): the order key of the s-mer that starts at every offset of the text"""
    n = len(seq)
    keys, valid = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=bool)
    spos = np_window_positions(seq, s)
    keys[spos] = order_keys(np_kmers(seq, s, canonical), hash_id, seed)
    valid[spos] = True
    return keys, valid


def kept_flags(seq, k, s, canonical, hash_id, seed):
    """-> (positions of ALL valid windows uint32, kept bool per window)"""
    seq = np.asarray(seq, dtype=np.uint8)
    assert 1 <= s <= min(k, 32)
    pos = np_window_positions(seq, k)
    if len(pos) == 0:
        return pos, np.zeros(0, dtype=bool)
    keys, valid = smer_keys(seq, s, canonical, hash_id, seed)
    span = k - s
    win = np.lib.stride_tricks.sliding_window_view(keys, span + 1)[pos]          # one row of k - s + 1 keys per valid window
    assert np.lib.stride_tricks.sliding_window_view(valid, span + 1)[pos].all()  # k valid bases: every s-mer inside is valid
    m = win.min(axis=1)
    return pos, (win[:, 0] == m) | (win[:, -1] == m)


def np_syncmers(seq, k, s, canonical, hash_id, seed, wide=False):
    """-> (k-mers uint64 (or (m, 2) for wide), positions uint32), ascending positions"""
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(seq, dtype=np.uint8)
    seq = np.asarray(seq, dtype=np.uint8)
    pos, keep = kept_flags(seq, k, s, canonical, hash_id, seed)
    km = np_kmers128(seq, k, canonical) if wide else np_kmers(seq, k, canonical)
    assert len(km) == len(pos)
    return km[keep], pos[keep]


def np_syncmers_fastq(text, k, s, canonical, hash_id, seed, wide=False):
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, dtype=np.uint8)
    return np_syncmers(fastq_masked(text), k, s, canonical, hash_id, seed, wide)


def _smer_of(v, k, s, j):
    return (v >> (2 * (k - s - j))) & ((1 << (2 * s)) - 1)


def _canon(x, s):
    rc = 0
    for j in range(s):
        rc |= (3 - ((x >> (2 * j)) & 3)) << (2 * (s - 1 - j))
    return min(x, rc)


def np_is_syncmer(keys, k, s, canonical, hash_id, seed):
    """the keep test on packed k-mers alone (uint64[n], or (n, 2) rows {w0, w1}): bool per key"""
    keys = np.asarray(keys, dtype=np.uint64)
    vals = [int(a) for a in keys] if keys.ndim == 1 else [int(a) | (int(b) << 64) for a, b in keys]
    if not vals:
        return np.zeros(0, dtype=bool)
    nj = k - s + 1
    sm = np.array([(_canon(_smer_of(v, k, s, j), s) if canonical else _smer_of(v, k, s, j)) & M64 for v in vals for j in range(nj)], dtype=np.uint64)
    h = order_keys(sm, hash_id, seed).reshape(len(vals), nj)
    m = h.min(axis=1)
    return (h[:, 0] == m) | (h[:, -1] == m)
