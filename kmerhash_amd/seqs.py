"""Text front ends of both key widths over the handle-free C calls: every k-mer of a text (kh_kmers_from_* / kh_kmers128_from_*), the
(w,k)-minimizers, the closed syncmers and the context-free syncmer test.  kmerhash_amd.kmers and kmerhash_amd.wide re-export them.

The k-mer definition is this library's (see kh_kmers_from_sequence in include/kmerhash_amd.h): 2-bit packed, first base most
significant, A=0 C=1 G=2 T=3, windows containing any other byte are skipped, canonical = min(k-mer, reverse complement).  A k-mer with
32 < k <= 64 is the 16-byte key {w0, w1} of kmerhash_amd.wide."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._call import _Buf, alloc, check, count_then_emit, stream_of
from .table import _hash_id


def _kmers(fn_name, words, seq, k, canonical, device, with_positions=False):
    """shared body of kmers_from_sequence / kmers128_from_sequence (and their FASTQ and position forms): `words` 64-bit words per k-mer;
    room for one k-mer per byte, cut to what came out"""
    b = _Buf.text(seq)
    room = max(b.n, 1)
    km, kptr = alloc(b, room if words == 1 else (room, words), np.uint64)
    n_out = C.c_uint64()
    if not with_positions:
        check(getattr(K.lib(), fn_name)(b.ptr, b.n, k, 1 if canonical else 0, b.where, kptr, C.byref(n_out), device, stream_of(b, device)), fn_name)
        return km[: n_out.value]
    pos, pptr = alloc(b, room, np.uint32)
    fn_name += "_pos"
    check(getattr(K.lib(), fn_name)(b.ptr, b.n, k, 1 if canonical else 0, b.where, kptr, pptr, C.byref(n_out), device, stream_of(b, device)), fn_name)
    return km[: n_out.value], pos[: n_out.value]


def kmers_from_fastq(text, k=31, canonical=True, device=0, with_positions=False):
    """raw FASTQ text (whole 4-line records; bytes / uint8 array on the host, or a uint8 CUDA tensor) -> packed k-mers of the
    sequence lines: the record structure is resolved on the GPU (kh_kmers_from_fastq), no host-side parsing.
    with_positions: -> (k-mers, byte offsets of their windows in the raw text)"""
    return kmers_from_sequence(text, k, canonical, device, _fastq=True, with_positions=with_positions)


def kmers_from_sequence(seq, k=31, canonical=True, device=0, _fastq=False, with_positions=False):
    """-> packed k-mers (numpy uint64 for host input, torch int64 CUDA tensor for device input), sequence order.
    with_positions: -> (k-mers, positions): positions[i] (numpy uint32 / torch int32) is the byte offset in `seq` of the first base
    of the window that gave k-mers[i] (kh_kmers_from_sequence_pos; a text of 2^32 bytes or more is refused)"""
    return _kmers("kh_kmers_from_fastq" if _fastq else "kh_kmers_from_sequence", 1, seq, k, canonical, device, with_positions)


def kmers128_from_sequence(seq, k=63, canonical=True, device=0, _fastq=False, with_positions=False):
    """-> (n, 2) k-mers (numpy uint64 for host input, torch int64 CUDA tensor for device input), sequence order; k = 1..64.
    with_positions: -> (k-mers, positions): positions[i] (numpy uint32 / torch int32) is the byte offset in `seq` of the first base of
    the window that gave k-mers[i] (a text of 2^32 bytes or more is refused)"""
    return _kmers("kh_kmers128_from_fastq" if _fastq else "kh_kmers128_from_sequence", 2, seq, k, canonical, device, with_positions)


def kmers128_from_fastq(text, k=63, canonical=True, device=0, with_positions=False):
    """raw FASTQ text (whole 4-line records) -> (n, 2) k-mers of the sequence lines (record structure resolved on the GPU);
    with_positions: -> (k-mers, byte offsets of their windows in the raw text)"""
    return kmers128_from_sequence(text, k, canonical, device, _fastq=True, with_positions=with_positions)


def _sampled(fn_name, words, seq, k, arg, canonical, order_hash, order_seed, device):
    """shared body of the samplers: `arg` is w of the minimizers, s of the syncmers"""
    return count_then_emit(fn_name, words, seq, (int(k), int(arg), 1 if canonical else 0, _hash_id(order_hash), int(order_seed)), device)


def minimizers_from_sequence(seq, k=15, w=10, canonical=True, order_hash="murmur", order_seed=42, device=0, _fastq=False):
    """(w,k)-minimizers of `seq` -> (k-mers, positions), ascending positions: of every w consecutive valid windows the one whose
    k-mer has the smallest order_hash(k-mer, order_seed) is kept (ties: the leftmost), each once -- about 2 / (w + 1) of the windows
    of kmers_from_sequence(with_positions=True), and all of them for w = 1 (kh_minimizers_from_sequence in include/kmerhash_amd.h).
    numpy uint64 / uint32 for host input, torch int64 / int32 CUDA tensors for device input.  A count pass first, then an exact
    allocation.  In a stretch of equal k-mers (poly-A) every full-window start is kept."""
    return _sampled("kh_minimizers_from_fastq" if _fastq else "kh_minimizers_from_sequence", 1, seq, k, w, canonical, order_hash, order_seed, device)


def minimizers_from_fastq(text, k=15, w=10, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """minimizers_from_sequence over the sequence lines of raw FASTQ text (whole 4-line records); positions are byte offsets into
    the text, no pick falls on an id or quality line and no window spans two reads"""
    return minimizers_from_sequence(text, k, w, canonical, order_hash, order_seed, device, _fastq=True)


def syncmers_from_sequence(seq, k=15, s=11, canonical=True, order_hash="murmur", order_seed=42, device=0, _fastq=False):
    """closed syncmers of `seq` -> (k-mers, positions), ascending positions: the windows of kmers_from_sequence(with_positions=True)
    whose smallest s-mer by order_hash(s-mer, order_seed) -- of the canonical s-mer when `canonical` -- is the first or the last of the
    k - s + 1 (kh_syncmers_from_sequence in include/kmerhash_amd.h).  About 2 / (k - s + 1) of the windows; all of them for s = k.
    Whether a k-mer is kept depends on the k-mer alone (is_syncmer asks without a text).  numpy uint64 / uint32 for host input, torch
    int64 / int32 CUDA tensors for device input.  In a homopolymer every window is kept."""
    return _sampled("kh_syncmers_from_fastq" if _fastq else "kh_syncmers_from_sequence", 1, seq, k, s, canonical, order_hash, order_seed, device)


def syncmers_from_fastq(text, k=15, s=11, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """syncmers_from_sequence over the sequence lines of raw FASTQ text (whole 4-line records); positions are byte offsets into the text"""
    return syncmers_from_sequence(text, k, s, canonical, order_hash, order_seed, device, _fastq=True)


def syncmers128_from_sequence(seq, k=63, s=31, canonical=True, order_hash="murmur", order_seed=42, device=0, _fastq=False):
    """closed syncmers of `seq` as 16-byte k-mers, k = 1..64, s = 1..min(k, 32) -> ((m, 2) k-mers, positions), ascending positions: the
    windows of kmers128_from_sequence(with_positions=True) whose smallest s-mer by order_hash (of the canonical s-mer when `canonical`)
    is the first or the last of the k - s + 1 (kh_syncmers128_from_sequence; kmerhash_amd.syncmers_from_sequence for the definition)"""
    return _sampled("kh_syncmers128_from_fastq" if _fastq else "kh_syncmers128_from_sequence", 2, seq, k, s, canonical, order_hash, order_seed, device)


def syncmers128_from_fastq(text, k=63, s=31, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """syncmers128_from_sequence over the sequence lines of raw FASTQ text (whole 4-line records); positions are byte offsets into the text"""
    return syncmers128_from_sequence(text, k, s, canonical, order_hash, order_seed, device, _fastq=True)


def _syncmer_mask(fn_name, words, keys, k, s, canonical, order_hash, order_seed, device):
    """shared body of is_syncmer / is_syncmer128: -> bool array / tensor, one entry per key"""
    kb = _Buf.keys(keys, words)
    mask, mptr = alloc(kb, kb.n, np.uint8, zero=True)
    check(getattr(K.lib(), fn_name)(kb.ptr, kb.n, int(k), int(s), 1 if canonical else 0, _hash_id(order_hash), int(order_seed), kb.where, mptr, device,
                                    stream_of(kb, device)), fn_name)
    return mask.bool() if kb.dev else mask.astype(bool)


def is_syncmer(keys, k=15, s=11, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """for packed k-mers (uint64 numpy array or int64 CUDA tensor): a bool array / tensor, True where the k-mer is a closed syncmer
    under these parameters -- the k-mers syncmers_from_sequence keeps, whatever text they stand in (kh_syncmer_mask)"""
    return _syncmer_mask("kh_syncmer_mask", 1, keys, k, s, canonical, order_hash, order_seed, device)


def is_syncmer128(keys, k=63, s=31, canonical=True, order_hash="murmur", order_seed=42, device=0):
    """for (n, 2) 16-byte k-mers: a bool array / tensor, True where the k-mer is a closed syncmer under these parameters (kh_wide_syncmer_mask)"""
    return _syncmer_mask("kh_wide_syncmer_mask", 2, keys, k, s, canonical, order_hash, order_seed, device)
