"""TEST HELPER: numpy model of (w,k)-minimizer sampling (kh_minimizers_from_sequence in include/kmerhash_amd.h).  The reference tree has
no sampler, so this model is the yardstick.  It is a direct statement of the definition: valid windows and k-mers from
oracle/kmers_np.py and tests/index_model.py (imported, not restated), order keys from the CPU hash oracle.oracle_py.hash_batch -- never
the GPU library's hash --, and for every full window np.argmin over its w keys (the first minimum = the leftmost), then the unique
of the picks."""
import numpy as np

from oracle import oracle_py as O
from oracle.kmers_np import np_kmers
from tests.index_model import fastq_masked, np_window_positions

HASH_IDS = {"identity": O.HASH_IDENTITY, "murmur3avx64": O.HASH_MURMUR3_X86, "murmur_x86": O.HASH_MURMUR3_X86, "murmur": O.HASH_MURMUR3_X64,
            "farm": O.HASH_FARM}


def order_keys(kmers, hash_id, seed):
    """h(p) of the emitted k-mers, by the CPU oracle"""
    hid = HASH_IDS[hash_id] if isinstance(hash_id, str) else int(hash_id)
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
    if len(kmers) == 0:
        return np.zeros(0, dtype=np.uint64)
    return np.asarray(O.hash_batch(hid, seed, kmers), dtype=np.uint64)


def np_minimizers(seq, k, w, canonical, hash_id, seed):
    """-> (k-mers uint64, positions uint32), ascending positions"""
    if isinstance(seq, (bytes, bytearray)):
        seq = np.frombuffer(seq, dtype=np.uint8)
    seq = np.asarray(seq, dtype=np.uint8)
    km, pos = np_kmers(seq, k, canonical), np_window_positions(seq, k)
    assert len(km) == len(pos)
    none = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    if len(km) < w:
        return none
    h = order_keys(km, hash_id, seed)
    # entry i of the valid windows starts a full window iff the next w - 1 valid windows sit at the next w - 1 offsets
    p64 = pos.astype(np.int64)
    full = np.nonzero(p64[w - 1:] - p64[: len(p64) - w + 1] == w - 1)[0]
    if len(full) == 0:
        return none
    win = np.lib.stride_tricks.sliding_window_view(h, w)[full]           # one row of w keys per full window
    picks = np.unique(full + np.argmin(win, axis=1))                     # argmin: the first of equal minima
    return km[picks], pos[picks]


def np_minimizers_fastq(text, k, w, canonical, hash_id, seed):
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(text, dtype=np.uint8)
    return np_minimizers(fastq_masked(text), k, w, canonical, hash_id, seed)
