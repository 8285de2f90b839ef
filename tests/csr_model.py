"""TEST HELPER: numpy model of kh_csr_unpermute (include/kmerhash_amd.h): a CSR given in a permuted order -- counts_perm[j] and the
j-th segment of pos_perm belong to query origin[j] -- put back into query order, by slicing."""
import numpy as np


def np_csr_unpermute(counts_perm, pos_perm, origin):
    """-> (counts uint32[n], offsets uint64[n + 1], positions uint32[total]) in query order"""
    counts_perm = np.asarray(counts_perm, dtype=np.uint32)
    pos_perm = np.asarray(pos_perm, dtype=np.uint32)
    origin = np.asarray(origin, dtype=np.int64)
    n = len(counts_perm)
    assert len(origin) == n and np.array_equal(np.sort(origin), np.arange(n)), "origin must be a permutation of 0..n-1"
    begin_perm = np.concatenate([[0], np.cumsum(counts_perm.astype(np.int64))])
    assert begin_perm[-1] == len(pos_perm)
    counts = np.zeros(n, dtype=np.uint32)
    counts[origin] = counts_perm
    slot_of = np.zeros(n, dtype=np.int64)
    slot_of[origin] = np.arange(n)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    parts = [pos_perm[begin_perm[j]: begin_perm[j + 1]] for j in slot_of if begin_perm[j + 1] > begin_perm[j]]
    pos = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)
    return counts, offsets, pos
