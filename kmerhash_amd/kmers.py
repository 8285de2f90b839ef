"""k-mer counting front end: the BenchmarkKmerCounter shape (BenchmarkKmerCounter.cpp:1476-1787: read
FASTQ/FASTA -> k-mers -> counting insert -> write (k-mer, count) tuples) on the GPU tables.

The reference takes its parser and k-mer type from kmerind (absent), so the k-mer definition here is this library's
(see kh_kmers_from_sequence in include/kmerhash_amd.h): 2-bit packed, first base most significant, A=0 C=1 G=2 T=3,
windows containing any other byte are skipped, canonical = min(k-mer, reverse complement)."""
import collections
import ctypes as C
import time

import numpy as np

from . import _capi as K
from ._call import _Buf, _is_tensor, alloc, check, check_same, stream_of, torch, two_pass
from .hll import estimate_average_per_rank, hyperloglog64
from .seqs import (is_syncmer, kmers128_from_fastq, kmers128_from_sequence, kmers_from_fastq, kmers_from_sequence,  # noqa: F401  (re-exported)
                   minimizers_from_fastq, minimizers_from_sequence, syncmers_from_fastq, syncmers_from_sequence)
from .table import hashmap_robinhood_doubling
from .targets import TARGET_NONE, Targets  # noqa: F401  (TARGET_NONE re-exported)
from .wide import hashmap_robinhood_doubling_wide


def sequences_from_fastq(buf):
    """FASTQ text (bytes / uint8 array) -> uint8 array holding only the sequence lines, each followed by '\\n'
    (records are 4 lines: @id, sequence, +, quality)."""
    raw = bytes(buf) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8).tobytes()
    seqs = raw.split(b"\n")[1::4]
    if not seqs:
        return np.zeros(0, dtype=np.uint8)
    return np.frombuffer(b"\n".join(seqs) + b"\n", dtype=np.uint8).copy()


def sequences_from_fasta(buf):
    """FASTA text -> sequence bytes; header lines are replaced by a single '\\n' so that k-mers never span records
    (line breaks inside a record are removed)."""
    a = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8)
    lines = bytes(a).split(b"\n")
    parts = []
    for ln in lines:
        if ln.startswith(b">"):
            parts.append(b"\n")
        else:
            parts.append(ln.strip())
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


POS_INVALID = 0xFFFFFFFF          # KH_POS_INVALID: the stamp of a window that is not k bases inside the text


def stamp_strand(text, pos, k, pos_base=0, device=0, count_invalid=False):
    """window positions -> stamped positions ((pos_base + p) << 1) | rc(p), where rc(p) = 1 iff the reverse complement of the k bases at
    text[p:p + k] is strictly smaller than the window: the case in which a canonical front end emitted the reverse complement
    (kh_stamp_strand in include/kmerhash_amd.h; a palindrome has rc = 0).  A window that passes the end of the text or holds a byte
    that is no base gives POS_INVALID.  Positions in any order, repeats allowed; k = 1..64; pos_base + len(text) <= 2^31.
    numpy uint8 / uint32 in, numpy uint32 out; CUDA tensors in (uint8 text, int32 positions), an int32 tensor out, queued on the current
    stream.  count_invalid: -> (stamped, number of POS_INVALID written), which waits for the stream."""
    tb, pb = _Buf.text(text), _Buf(pos, np.uint32)
    check_same("text and positions must live in the same memory", tb, pb, length=False)
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be 1..64, got %r" % (k,))
    if not 0 <= int(pos_base) or int(pos_base) + tb.n > 2 ** 31:
        raise ValueError("pos_base + len(text) must stay within 2^31 (a stamped position has 31 bits), got %r + %d" % (pos_base, tb.n))
    out, optr = alloc(pb, pb.n, np.uint32)
    bad = C.c_uint64()
    check(K.lib().kh_stamp_strand(tb.ptr, tb.n, int(k), pb.ptr, pb.n, int(pos_base), pb.where, optr, C.byref(bad) if count_invalid else None, device,
                                  stream_of(pb, device)), "kh_stamp_strand")
    return (out, bad.value) if count_invalid else out


def unstamp(v):
    """stamped positions -> (positions, strand bits): v >> 1 and v & 1 (numpy uint32 or int32 CUDA tensors holding uint32; POS_INVALID is
    the caller's to filter)"""
    if _is_tensor(v):
        return (v >> 1) & 0x7FFFFFFF, v & 1
    v = np.asarray(v, dtype=np.uint32)
    return v >> np.uint32(1), v & np.uint32(1)


def anchors_from_csr(qpos, offsets, pos, device=0):
    """the CSR of a find over a stranded index (stamped query positions, offsets, stamped hits) -> (qpos, rpos, rev) with one entry per hit
    (kh_anchors_from_csr): rev = 0 where the reference window equals the query window, 1 where it is its reverse complement"""
    qb, ob, pb = _Buf(qpos, np.uint32), _Buf(offsets, np.uint64), _Buf(pos, np.uint32)
    msg = "qpos, offsets (len(qpos) + 1 entries) and pos must live in the same memory"
    check_same(msg, qb, ob, pb, length=False)
    if ob.n != qb.n + 1:
        raise ValueError(msg)
    (oq, qptr), (orp, rptr), (orv, vptr) = alloc(pb, pb.n, np.uint32), alloc(pb, pb.n, np.uint32), alloc(pb, pb.n, np.uint8)
    check(K.lib().kh_anchors_from_csr(qb.ptr, ob.ptr, qb.n, pb.ptr, pb.n, qb.where, qptr, rptr, vptr, device, stream_of(qb, device)), "kh_anchors_from_csr")
    return oq, orp, orv


Chains = collections.namedtuple("Chains", "score pred chain first last count cscore")


def _check_chain_params(k, lookback, max_gap, band, min_score, min_count):
    """the refusals of kh_chain_anchors that depend on the parameters alone, as ValueError"""
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be 1..64, got %r" % (k,))
    if not 1 <= int(lookback) <= 64:
        raise ValueError("lookback must be 1..64 (the candidates of an anchor are scored by one wavefront), got %r" % (lookback,))
    if not 1 <= int(max_gap) <= 2 ** 31 - 1:
        raise ValueError("max_gap must be 1..2^31-1, got %r" % (max_gap,))
    if not 0 <= int(band) <= 2 ** 31 - 1:
        raise ValueError("band must be 0..2^31-1, got %r" % (band,))
    if not -2 ** 31 <= int(min_score) < 2 ** 31:
        raise ValueError("min_score must fit a signed 32-bit integer, got %r" % (min_score,))
    if not 0 <= int(min_count) < 2 ** 32:
        raise ValueError("min_count must be 0..2^32-1, got %r" % (min_count,))


def chain_anchors(qpos, rpos, rev, k, seg_offsets=None, lookback=64, max_gap=5000, band=500, min_score=40, min_count=3, device=0):
    """collinear chains of oriented anchors (kh_chain_anchors in include/kmerhash_amd.h, which holds the definition): per segment -- the
    anchors [seg_offsets[s], seg_offsets[s + 1]), one read; None: all of them -- a banded DP over the `lookback` anchors before each one,
    a partition of the anchors into disjoint chains and the chains with score >= min_score and count >= min_count, numbered by their
    first anchor.  -> Chains(score, pred, chain, first, last, count, cscore): f(i), pred(i) (-1: none) and the chain number (-1: not
    kept) per anchor, then first / last anchor, anchor count and score per kept chain.  numpy in (uint32, uint32, uint8, uint64), numpy
    out; CUDA tensors in (int32, int32, uint8, int64), tensors out on the current stream.  At most 2^24 anchors per call."""
    _check_chain_params(k, lookback, max_gap, band, min_score, min_count)
    qb, rb, vb = _Buf(qpos, np.uint32), _Buf(rpos, np.uint32), _Buf(rev, np.uint8)
    sb = None if seg_offsets is None else _Buf(seg_offsets, np.uint64)
    check_same("qpos, rpos, rev and seg_offsets must live in the same memory", qb, rb, vb, sb, length=False)
    m = qb.n
    if rb.n != m or vb.n != m:
        raise ValueError("qpos, rpos and rev must have one entry per anchor, got %d, %d and %d" % (m, rb.n, vb.n))
    if m > 2 ** 24:
        raise ValueError("at most 2^24 anchors per call (batch over reads), got %d" % m)
    if sb is not None and (sb.n < 1 or sb.n - 1 > m + 2 ** 24 or (sb.n == 1 and m)):
        raise ValueError("seg_offsets must hold n_seg + 1 entries ascending from 0 to the number of anchors, got %d entries for %d anchors" % (sb.n, m))
    cap = m // max(1, int(min_count))          # kept chains are disjoint and hold min_count anchors each
    # score, pred and chain per anchor (int32), then first, last, count (uint32) and score (int32) per kept chain
    outs = [alloc(qb, size, dt, empty=True) for size, dt in [(m, np.int32)] * 3 + [(cap, np.uint32)] * 3 + [(cap, np.int32)]]
    n = C.c_uint64()
    st = K.lib().kh_chain_anchors(qb.ptr_or_null, rb.ptr_or_null, vb.ptr_or_null, m, None if sb is None else sb.ptr,
                                  0 if sb is None else sb.n - 1, int(k), int(lookback), int(max_gap), int(band), int(min_score), int(min_count), qb.where,
                                  *(ptr for _, ptr in outs), cap, C.byref(n), device, stream_of(qb, device))
    check(st, "kh_chain_anchors" + (": seg_offsets do not ascend from 0 to the number of anchors" if st == K.KH_ERR_INVALID else ""))
    return Chains(*(a for a, _ in outs[:3]), *(a[:n.value] for a, _ in outs[3:]))


AnchorGroups = collections.namedtuple("AnchorGroups", "qpos rpos rev tid src offsets seg target")


def group_anchors(qpos, rpos, rev, targets, k, seg_offsets=None, device=0):
    """the anchors of every segment (read) regrouped by the target (contig) they fall in (kh_anchor_targets in include/kmerhash_amd.h,
    which holds the definition).  targets: a kmerhash_amd.Targets, or a (starts, ends) pair of arrays that live where the anchors live;
    an anchor belongs to target t iff its k bases lie inside [starts[t], ends[t]), to none (TARGET_NONE, 0xFFFFFFFF) otherwise.
    -> AnchorGroups(qpos, rpos, rev, tid, src, offsets, seg, target): the anchors sorted by (segment, target, input index) with their
    target ids and input indices (rpos = POS_INVALID where the id is TARGET_NONE: the chaining DP skips such an anchor), then the group
    CSR -- group g is the anchors [offsets[g], offsets[g + 1]), all of segment seg[g] and target target[g].  Hand `offsets` to
    chain_anchors as its seg_offsets and no chain crosses a target.  numpy in, numpy out (uint32, uint32, uint8, uint32, uint32, uint64,
    uint32, uint32); CUDA tensors in, tensors out on the current stream (int32 holding the uint32 bits, int64 offsets); the call waits for
    the stream once, to learn the number of groups.  At most 2^24 anchors and 2^24 targets per call."""
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be 1..64, got %r" % (k,))
    qb, rb, vb = _Buf(qpos, np.uint32), _Buf(rpos, np.uint32), _Buf(rev, np.uint8)
    sb = None if seg_offsets is None else _Buf(seg_offsets, np.uint64)
    if isinstance(targets, Targets):
        starts, ends = targets.to(qb.device) if qb.dev else (targets.starts, targets.ends)
    else:
        starts, ends = targets
    tsb, teb = _Buf(starts, np.uint32), _Buf(ends, np.uint32)
    check_same("qpos, rpos, rev, seg_offsets and the target table must live in the same memory", qb, rb, vb, sb, tsb, teb, length=False)
    m = qb.n
    if rb.n != m or vb.n != m:
        raise ValueError("qpos, rpos and rev must have one entry per anchor, got %d, %d and %d" % (m, rb.n, vb.n))
    if m > 2 ** 24:
        raise ValueError("at most 2^24 anchors per call (batch over reads), got %d" % m)
    if not 1 <= tsb.n <= 2 ** 24 or teb.n != tsb.n:
        raise ValueError("the target table must hold 1..2^24 targets, one start and one end each, got %d and %d" % (tsb.n, teb.n))
    if sb is not None and (sb.n < 1 or sb.n - 1 > m + 2 ** 24 or (sb.n == 1 and m)):
        raise ValueError("seg_offsets must hold n_seg + 1 entries ascending from 0 to the number of anchors, got %d entries for %d anchors" % (sb.n, m))
    outs = [alloc(qb, m, dt, empty=True) for dt in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32)]
    offs, optr = alloc(qb, m + 1, np.uint64, zero=not m)
    (gseg, sptr), (gtid, tptr) = alloc(qb, m, np.uint32, empty=True), alloc(qb, m, np.uint32, empty=True)
    n = C.c_uint64()
    if m:
        st = K.lib().kh_anchor_targets(qb.ptr, rb.ptr, vb.ptr, m, None if sb is None else sb.ptr, 0 if sb is None else sb.n - 1, tsb.ptr, teb.ptr, tsb.n, int(k),
                                       qb.where, *(p for _, p in outs), optr, sptr, tptr, C.byref(n), device, stream_of(qb, device))
        check(st, "kh_anchor_targets" + (": seg_offsets do not ascend from 0 to the number of anchors" if st == K.KH_ERR_INVALID else ""))
    g = n.value
    return AnchorGroups(*(a for a, _ in outs), offs[:g + 1], gseg[:g], gtid[:g])


ChainEdits = collections.namedtuple("ChainEdits", "link edits over")
EDITS_NOLINK, EDITS_OVER = -1, -2      # KH_EDITS_NOLINK, KH_EDITS_OVER


def _check_text_limits(k, m, tq, tr, ref_base):
    """what chain_edits, chain_cigars and chain_ends ask of k, the number of anchors and the two texts"""
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be 1..64, got %r" % (k,))
    if m > 2 ** 24:
        raise ValueError("at most 2^24 anchors per call (batch over reads), got %d" % m)
    if tq.n >= 2 ** 31:
        raise ValueError("the query text must be shorter than 2^31 bytes, got %d" % tq.n)
    if not 0 <= int(ref_base) or int(ref_base) + tr.n > 2 ** 31:
        raise ValueError("ref_base + len(rtext) must stay within 2^31 (a position has 31 bits), got %r + %d" % (ref_base, tr.n))


def chain_edits(qtext, rtext, qpos, rpos, rev, pred, chain, n_chains, k, ref_base=0, max_edits=31, device=0):
    """edit distance of every chain link against the two texts (kh_chain_edits in include/kmerhash_amd.h, which holds the definition):
    anchor i with pred[i] in the same kept chain is a link, A = qtext[q_pred, q_i) and B = the stretch of rtext it faces (rtext covers the
    reference coordinates [ref_base, ref_base + len(rtext)); reverse-strand links read it as its reverse complement).  pred and chain are
    those of chain_anchors, n_chains the number of its kept chains.  -> ChainEdits(link, edits, over): link[i] = the Levenshtein distance
    of the link, -1 (EDITS_NOLINK) where i has none, -2 (EDITS_OVER) where it leaves the texts or needs more than max_edits (0..31)
    edits; edits[c] = the sum of chain c's distances, over[c] = the number of its -2 links.  numpy in (uint8 / bytes, uint32, uint32,
    uint8, int32, int32), numpy out (int32, uint32, uint32); CUDA tensors in, int32 tensors out on the current stream, without a wait.
    At most 2^24 anchors per call."""
    if not 0 <= int(max_edits) <= 31:
        raise ValueError("max_edits must be 0..31 (one diagonal per lane of a wavefront), got %r" % (max_edits,))
    if not 0 <= int(n_chains) <= 2 ** 31:
        raise ValueError("n_chains must be 0..2^31, got %r" % (n_chains,))
    tq, tr = _Buf.text(qtext), _Buf.text(rtext)
    qb, rb, vb = _Buf(qpos, np.uint32), _Buf(rpos, np.uint32), _Buf(rev, np.uint8)
    pb, cb = _Buf(pred, np.int32), _Buf(chain, np.int32)
    check_same("the texts, qpos, rpos, rev, pred and chain must live in the same memory", tq, tr, qb, rb, vb, pb, cb, length=False)
    m, nc = qb.n, int(n_chains)
    check_same("qpos, rpos, rev, pred and chain must have one entry per anchor, got %d, %d, %d, %d and %d" % (m, rb.n, vb.n, pb.n, cb.n), qb, rb, vb, pb, cb)
    _check_text_limits(k, m, tq, tr, ref_base)
    (link, lptr), (edits, eptr), (over, optr) = (alloc(qb, size, dt, empty=True) for size, dt in ((m, np.int32), (nc, np.uint32), (nc, np.uint32)))
    if m or nc:
        check(K.lib().kh_chain_edits(tq.ptr_or_null, tq.n, tr.ptr_or_null, tr.n, int(ref_base), *(b.ptr_or_null for b in (qb, rb, vb, pb, cb)), m, nc, int(k),
                                     int(max_edits), qb.where, lptr, eptr, optr, device, stream_of(qb, device)), "kh_chain_edits")
    return ChainEdits(link, edits, over)


ChainCigars = collections.namedtuple("ChainCigars", "offsets ops ins dels")
CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}      # the BAM operation codes kh_chain_cigars writes: a run is (len << 4) | op


def chain_cigars(qtext, rtext, qpos, rpos, rev, pred, chain, n_chains, k, link, ref_base=0, device=0):
    """which edits chain_edits counted (kh_chain_cigars in include/kmerhash_amd.h, which holds the definition): per anchor link a
    run-length alignment of A = qtext[q_pred, q_i) against B = the stretch of rtext it faces, found by the traceback of the same
    furthest-reaching-point pass.  The inputs are those of chain_edits plus `link`, the array that call returned over them.
    -> ChainCigars(offsets, ops, ins, dels): a CSR in anchor order -- row i is ops[offsets[i]:offsets[i + 1]], each run (len << 4) | op
    with I = 1 (a base of A that B lacks), D = 2, '=' = 7 and X = 8; empty where i has no link, where the link is outside the texts or
    link[i] is not its distance -- then ins[c] and dels[c], the I and D bases of chain c.  Count, then emit: two calls, one allocation of
    the exact size.  numpy in, numpy out (uint64, uint32, uint32, uint32); CUDA tensors in, tensors out on the current stream (int64, then
    int32 holding the uint32 bits); the call waits for the stream once per pass, to learn the number of runs.  At most 2^24 anchors per
    call.  cigar_string() turns the rows of one chain into text."""
    if not 0 <= int(n_chains) <= 2 ** 31:
        raise ValueError("n_chains must be 0..2^31, got %r" % (n_chains,))
    tq, tr = _Buf.text(qtext), _Buf.text(rtext)
    qb, rb, vb = _Buf(qpos, np.uint32), _Buf(rpos, np.uint32), _Buf(rev, np.uint8)
    pb, cb, lb = _Buf(pred, np.int32), _Buf(chain, np.int32), _Buf(link, np.int32)
    check_same("the texts, qpos, rpos, rev, pred, chain and link must live in the same memory", tq, tr, qb, rb, vb, pb, cb, lb, length=False)
    m, nc = qb.n, int(n_chains)
    check_same("qpos, rpos, rev, pred, chain and link must have one entry per anchor, got %d, %d, %d, %d, %d and %d" % (m, rb.n, vb.n, pb.n, cb.n, lb.n),
               qb, rb, vb, pb, cb, lb)
    _check_text_limits(k, m, tq, tr, ref_base)
    (offs, optr), (ins, iptr), (dels, dptr) = alloc(qb, m + 1, np.uint64, zero=True), alloc(qb, nc, np.uint32, empty=True), alloc(qb, nc, np.uint32, empty=True)
    if m == 0 and (nc == 0 or not qb.dev):      # nothing to queue: the zeroed host arrays are the answer
        return ChainCigars(offs, alloc(qb, 0, np.uint32)[0], ins, dels)
    args = (tq.ptr_or_null, tq.n, tr.ptr_or_null, tr.n, int(ref_base), *(b.ptr_or_null for b in (qb, rb, vb, pb, cb)), m, nc, int(k), lb.ptr_or_null, qb.where, optr)
    return ChainCigars(offs, two_pass("kh_chain_cigars", args, qb, np.uint32, device, trail=(iptr, dptr)), ins, dels)


def _host(x, dtype):
    return (x.cpu().numpy() if _is_tensor(x) else np.asarray(x)).view(dtype) if len(x) else np.zeros(0, dtype=dtype)


def cigar_string(cigars, table, row, k):
    """the CIGAR of chain `row` of a ChainTable as text (a host helper: the arrays are copied to the host if they are tensors): the rows
    of the chain's anchors in ascending anchor order, then k '=' for its last seed, equal neighbours merged -- the query interval
    [q_start, q_end) against the reference interval [r_start, r_end), reverse-complemented for a reverse-strand chain.  None where a
    link of the chain has an empty row (outside the texts or more than max_edits: over[row] > 0 is the usual case): such a chain has no
    whole-chain alignment."""
    offs, ops, chain = _host(cigars.offsets, np.int64), _host(cigars.ops, np.uint32), _host(table.chain, np.int32)
    members = np.flatnonzero(chain == int(row))
    if members.size == 0:
        raise ValueError("chain %r has no anchors in this table" % (row,))
    runs = []
    for i in members[1:]:
        if offs[i + 1] == offs[i]:
            return None
        runs.extend((int(v) & 15, int(v) >> 4) for v in ops[offs[i]:offs[i + 1]])
    runs.append((7, int(k)))
    out = []
    for op, n in runs:
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return "".join("%d%s" % (n, CIGAR_OPS[op]) for op, n in out)


ChainEnds = collections.namedtuple("ChainEnds", "q r edits clip offsets ops")


def chain_ends(qtext, rtext, qpos, rpos, rev, first, last, q_lo, q_hi, k, ref_base=0, max_edits=31, clip_cost=4, device=0):
    """both ends of every chain, extended from its outermost seeds to the ends of its read or to a soft clip (kh_chain_ends in
    include/kmerhash_amd.h, which holds the definition).  first / last: the anchor indices of each chain's first and last anchor
    (Chains.first / .last of chain_anchors); q_lo / q_hi: the byte interval [q_lo, q_hi) of the chain's read in qtext.  Row 2c is the head
    of chain c (the read's bases before its first seed), row 2c + 1 its tail (those behind its last seed); an end stops at the point of
    greatest (aligned read bases - clip_cost * edits) among at most max_edits (0..31) edits, clip_cost 1..255.
    -> ChainEnds(q, r, edits, clip, offsets, ops): per row the read bases aligned, the reference bases they face, the edits, and the read
    bases left over (the soft clip); then a CSR of runs (len << 4) | op as chain_cigars writes them, a head's row in read order.  Count,
    then emit: two calls, one allocation of the exact size.  numpy in, numpy out (uint32 x 4, uint64, uint32); CUDA tensors in, tensors out
    on the current stream (int32 holding the uint32 bits, int64 offsets); the call waits for the stream once per pass, to learn the number
    of runs.  At most 2^24 anchors and 2^23 chains per call.  read_cigar() and extended_intervals() put the ends onto a ChainTable."""
    if not 0 <= int(max_edits) <= 31:
        raise ValueError("max_edits must be 0..31 (one diagonal per lane of a wavefront), got %r" % (max_edits,))
    if not 1 <= int(clip_cost) <= 255:
        raise ValueError("clip_cost must be 1..255, got %r" % (clip_cost,))
    tq, tr = _Buf.text(qtext), _Buf.text(rtext)
    qb, rb, vb = _Buf(qpos, np.uint32), _Buf(rpos, np.uint32), _Buf(rev, np.uint8)
    fb, lb, ob, hb = _Buf(first, np.uint32), _Buf(last, np.uint32), _Buf(q_lo, np.uint32), _Buf(q_hi, np.uint32)
    check_same("the texts, qpos, rpos, rev, first, last, q_lo and q_hi must live in the same memory", tq, tr, qb, rb, vb, fb, lb, ob, hb, length=False)
    m, nc = qb.n, fb.n
    check_same("qpos, rpos and rev must have one entry per anchor, got %d, %d and %d" % (m, rb.n, vb.n), qb, rb, vb)
    check_same("first, last, q_lo and q_hi must have one entry per chain, got %d, %d, %d and %d" % (nc, lb.n, ob.n, hb.n), fb, lb, ob, hb)
    _check_text_limits(k, m, tq, tr, ref_base)
    if nc > 2 ** 23:
        raise ValueError("at most 2^23 chains per call (batch over reads), got %d" % nc)
    nums = [alloc(fb, 2 * nc, np.uint32, empty=True) for _ in range(4)]
    offs, optr = alloc(fb, 2 * nc + 1, np.uint64, zero=True)
    if nc == 0:      # nothing to queue: the zeroed offset is the answer
        return ChainEnds(*(a for a, _ in nums), offs, alloc(fb, 0, np.uint32)[0])
    args = (tq.ptr_or_null, tq.n, tr.ptr_or_null, tr.n, int(ref_base), qb.ptr_or_null, rb.ptr_or_null, vb.ptr_or_null, m, fb.ptr, lb.ptr, ob.ptr, hb.ptr, nc,
            int(k), int(max_edits), int(clip_cost), fb.where, *(p for _, p in nums), optr)
    return ChainEnds(*(a for a, _ in nums), offs, two_pass("kh_chain_ends", args, fb, np.uint32, device))


ChainSelect = collections.namedtuple("ChainSelect", "parent rank mapq flag sub nsub best")
FLAG_PRIMARY, FLAG_KEPT = 1, 2      # the bits of ChainSelect.flag


def _check_select_params(mask_pct, pri_pct, best_n):
    """the refusals of kh_chain_select that depend on the parameters alone, as ValueError"""
    if not 0 <= int(mask_pct) <= 100:
        raise ValueError("mask_pct must be 0..100, got %r" % (mask_pct,))
    if not 0 <= int(pri_pct) <= 100:
        raise ValueError("pri_pct must be 0..100, got %r" % (pri_pct,))
    if not 0 <= int(best_n) < 2 ** 32:
        raise ValueError("best_n must be 0..2^32-1, got %r" % (best_n,))


def select_chains(q_start, q_end, score, count, read_offsets=None, mask_pct=50, pri_pct=80, best_n=5, device=0):
    """which chain of every read is the answer, and how sure (kh_chain_select in include/kmerhash_amd.h, which holds the definition): per
    group -- the chains [read_offsets[g], read_offsets[g + 1]), one read; None: all of them -- the chains in order of score (ties: the
    smaller number); a chain is secondary when an earlier primary covers mask_pct % of the shorter of the two query intervals, else
    primary; a primary gets a mapping quality 0..60 from the score gap to its best secondary, its anchor count and its score.
    -> ChainSelect(parent, rank, mapq, flag, sub, nsub, best): per chain the chain number of its primary (its own for a primary), its
    rank in the group, the mapping quality (0 for a secondary), flag bit 0 = primary and bit 1 = kept (a primary; a secondary with
    100 * score >= pri_pct * its parent's that is among the first best_n of its parent), and for a primary the best secondary score and
    the number of secondaries; per group the chain of rank 0, -1 for a read without chains.  numpy in (uint32, uint32, int32, uint32,
    uint64), numpy out (int32, uint32, uint8, uint8, int32, uint32, int32); CUDA tensors in (int32 x 4, int64), tensors out on the current
    stream (int32 holding the uint32 bits) -- queued only: the call does not wait for the stream.  At most 2^23 chains per call."""
    _check_select_params(mask_pct, pri_pct, best_n)
    sb, eb, cb, nb = _Buf(q_start, np.uint32), _Buf(q_end, np.uint32), _Buf(score, np.int32), _Buf(count, np.uint32)
    ob = None if read_offsets is None else _Buf(read_offsets, np.uint64)
    check_same("q_start, q_end, score, count and read_offsets must live in the same memory", sb, eb, cb, nb, ob, length=False)
    n = sb.n
    check_same("q_start, q_end, score and count must have one entry per chain, got %d, %d, %d and %d" % (n, eb.n, cb.n, nb.n), sb, eb, cb, nb)
    if n > 2 ** 23:
        raise ValueError("at most 2^23 chains per call (batch over reads), got %d" % n)
    if ob is not None and (ob.n < 2 or ob.n - 1 > n + 2 ** 24):
        raise ValueError("read_offsets must hold n_reads + 1 >= 2 entries ascending from 0 to the number of chains, got %d entries for %d chains" % (ob.n, n))
    ng = 1 if ob is None else ob.n - 1
    outs = [alloc(sb, n, dt, empty=True) for dt in (np.int32, np.uint32, np.uint8, np.uint8, np.int32, np.uint32)]
    best, bptr = alloc(sb, ng, np.int32)
    # (no chains in host memory: the call answers without a device)
    st = K.lib().kh_chain_select(sb.ptr_or_null, eb.ptr_or_null, cb.ptr_or_null, nb.ptr_or_null, n, None if ob is None else ob.ptr, 0 if ob is None else ng,
                                 int(mask_pct), int(pri_pct), int(best_n), sb.where, *(p for _, p in outs), bptr, device, stream_of(sb, device))
    check(st, "kh_chain_select" + (": read_offsets do not ascend from 0 to the number of chains" if st == K.KH_ERR_INVALID else ""))
    return ChainSelect(*(a for a, _ in outs), best)


def select_table(table, n_reads=None, **params):
    """select_chains over the rows of a ChainTable (index.chains): the groups are the runs of equal table.seg, which does not descend.
    n_reads: the number of reads (default: the last seg + 1, 0 for an empty table); a read without chains gets best == -1.
    params: mask_pct, pri_pct, best_n, device."""
    seg = table.seg
    dev = _is_tensor(seg) and seg.is_cuda
    rows = int(seg.numel() if _is_tensor(seg) else len(seg))
    if n_reads is None:
        n_reads = int(seg.max()) + 1 if rows else 0
    n_reads = int(n_reads)
    if n_reads < 0 or (rows and n_reads == 0):
        raise ValueError("n_reads must cover the reads of the table, got %r" % (n_reads,))
    if n_reads == 0:               # an empty table of no reads: nothing to select, no group to report
        _check_select_params(params.get("mask_pct", 50), params.get("pri_pct", 80), params.get("best_n", 5))
        like = _Buf(table.score, np.int32)
        return ChainSelect(*(alloc(like, 0, dt)[0] for dt in (np.int32, np.uint32, np.uint8, np.uint8, np.int32, np.uint32, np.int32)))
    # read g owns the rows with seg == g: offsets[g] = the first row with seg >= g
    if dev:
        offs = torch.searchsorted(seg.long(), torch.arange(n_reads + 1, dtype=torch.int64, device=seg.device))
    else:
        offs = np.searchsorted(np.asarray(seg).astype(np.int64), np.arange(n_reads + 1, dtype=np.int64), side="left").astype(np.uint64)
    if int(offs[-1]) != rows:
        raise ValueError("n_reads = %d does not cover the reads of the table (seg reaches %d)" % (n_reads, int(seg.max())))
    return select_chains(table.q_start, table.q_end, table.score, table.count, offs, **params)


PairSelect = collections.namedtuple("PairSelect", "row mapq tlen flag score nconc")
PAIR_PROPER, PAIR_BOTH, PAIR_SAME_TARGET = 1, 2, 4      # the bits of PairSelect.flag


def _check_pair_params(min_ins, max_ins, unpaired_pen):
    """the refusals of kh_pair_chains that depend on the parameters alone, as ValueError"""
    if not 0 <= int(min_ins) <= int(max_ins) < 2 ** 32:
        raise ValueError("0 <= min_ins <= max_ins < 2^32 is needed, got %r and %r" % (min_ins, max_ins))
    if not 0 <= int(unpaired_pen) < 2 ** 32:
        raise ValueError("unpaired_pen must be 0..2^32-1, got %r" % (unpaired_pen,))


def pair_chains(rs, re, rev, score, read_offsets, tid=None, use=None, mapq=None, min_ins=0, max_ins=1000, unpaired_pen=17, device=0):
    """the chain rows of the two mates of every read pair, looked at together (kh_pair_chains in include/kmerhash_amd.h, which holds the
    definition).  Reads 2p and 2p + 1 are mate 1 and mate 2 of pair p; read s owns the chains [read_offsets[s], read_offsets[s + 1]).
    Per chain: the reference interval [rs, re), the strand rev, the score, and optionally its target number tid (None: one target), use
    (non-zero: a candidate; None: all) and the single-read quality mapq (None: 0).  A combination of one candidate per mate is
    concordant when both lie on one target, on opposite strands, forward before reverse, with a fragment length re_reverse - rs_forward
    in [min_ins, max_ins]; the pair is proper when the best concordant pair score + unpaired_pen reaches the sum of the two best single
    scores.  Only the 64 best candidates of a mate take part.
    -> PairSelect(row, mapq, tlen, flag, score, nconc): per read the chain that represents it (-1: none), its quality -- for a proper
    pair raised to 60 * (1 - best other pair score / pair score) where that is more -- and the signed template length; per pair flag
    bit 0 = proper, bit 1 = both mates have a row, bit 2 = the rows share a target, the best concordant pair score and the number of
    concordant combinations.  numpy in (uint32, uint32, uint8, int32, uint64; uint32, uint8, uint8), numpy out (int32, uint8, int32,
    uint8, int32, uint32); CUDA tensors in, tensors out on the current stream -- queued only: the call does not wait for the stream.
    At most 2^23 chains per call."""
    _check_pair_params(min_ins, max_ins, unpaired_pen)
    sb, eb, vb, cb, ob = _Buf(rs, np.uint32), _Buf(re, np.uint32), _Buf(rev, np.uint8), _Buf(score, np.int32), _Buf(read_offsets, np.uint64)
    tb = None if tid is None else _Buf(tid, np.uint32)
    ub = None if use is None else _Buf(use, np.uint8)
    mb = None if mapq is None else _Buf(mapq, np.uint8)
    check_same("rs, re, rev, score, read_offsets, tid, use and mapq must live in the same memory", sb, eb, vb, cb, ob, tb, ub, mb, length=False)
    n = sb.n
    check_same("rs, re, rev, score, tid, use and mapq must have one entry per chain", sb, eb, vb, cb, tb, ub, mb)
    if n > 2 ** 23:
        raise ValueError("at most 2^23 chains per call (batch over reads), got %d" % n)
    if ob.n < 1 or ob.n - 1 > n + 2 ** 24:
        raise ValueError("read_offsets must hold n_reads + 1 entries ascending from 0 to the number of chains, got %d entries for %d chains" % (ob.n, n))
    n_reads = ob.n - 1
    if n_reads % 2:
        raise ValueError("reads come in pairs (mate 1, mate 2, ...): an even number of reads is needed, got %d" % n_reads)
    per_read = [alloc(ob, n_reads, dt, empty=True) for dt in (np.int32, np.uint8, np.int32)]
    per_pair = [alloc(ob, n_reads // 2, dt, empty=True) for dt in (np.uint8, np.int32, np.uint32)]
    opt = lambda b: None if b is None else b.ptr_or_null      # noqa: E731
    st = K.lib().kh_pair_chains(sb.ptr_or_null, eb.ptr_or_null, vb.ptr_or_null, cb.ptr_or_null, opt(tb), opt(ub), opt(mb), n, ob.ptr, n_reads,
                                int(min_ins), int(max_ins), int(unpaired_pen), ob.where, *(p for _, p in per_read + per_pair), device, stream_of(ob, device))
    check(st, "kh_pair_chains" + (": read_offsets do not ascend from 0 to the number of chains" if st == K.KH_ERR_INVALID else ""))
    return PairSelect(*(a for a, _ in per_read + per_pair))


def pair_mapping(mapping, n_reads, targets=None, **params):
    """pair_chains over the rows of a Mapping (index.map) whose reads are interleaved mate 1, mate 2, ...: a row is a candidate when
    select kept it and records.valid says it has a whole alignment -- and, with targets (the kmerhash_amd.Targets the Mapping was made
    with), when its interval lies inside one target: the printable rule of write_paf.  The intervals are records.rs / records.re, the
    strand table.rev, the score table.score, the quality select.mapq, the target targets.locate(records.rs), the CSR the runs of equal
    table.seg as select_table() makes it.  params: min_ins, max_ins, unpaired_pen, device.  -> PairSelect
    n_reads must cover the reads of the table.  A numpy Mapping is checked (ValueError); a tensor Mapping is not, because the check would
    be a host wait: rows of reads at or beyond n_reads then fall outside the CSR and take no part, silently."""
    n_reads = int(n_reads)
    if n_reads < 0 or n_reads % 2:
        raise ValueError("reads come in pairs (mate 1, mate 2, ...): an even number of reads is needed, got %r" % (n_reads,))
    t, sel, rec = mapping.table, mapping.select, mapping.records
    seg = t.seg
    dev = _is_tensor(seg) and seg.is_cuda
    rows = int(seg.numel() if _is_tensor(seg) else len(seg))
    tid = None
    if dev:
        offs = torch.searchsorted(seg.long(), torch.arange(n_reads + 1, dtype=torch.int64, device=seg.device))
        use = ((sel.flag & FLAG_KEPT) != 0) & (rec.valid != 0)
        if targets is not None:
            tgt, _ = targets.locate(rec.rs)
            ends = targets.to(seg.device)[1].long() & 0xFFFFFFFF
            use = use & (tgt >= 0) & ((rec.re.long() & 0xFFFFFFFF) <= ends[tgt.clamp(min=0)])
            tid = tgt.int()      # (-1 holds the bits of KH_TARGET_NONE)
        use = use.to(torch.uint8)
    else:
        sg = np.asarray(seg).astype(np.int64)
        offs = np.searchsorted(sg, np.arange(n_reads + 1, dtype=np.int64), side="left").astype(np.uint64)
        if int(offs[-1]) != rows:
            raise ValueError("n_reads = %d does not cover the reads of the table (seg reaches %d)" % (n_reads, int(sg.max())))
        use = ((_host(sel.flag, np.uint8) & FLAG_KEPT) != 0) & (_host(rec.valid, np.uint8) != 0)
        if targets is not None:
            tgt, _ = targets.locate(_host(rec.rs, np.uint32))
            use = use & (tgt >= 0) & (_host(rec.re, np.uint32).astype(np.int64) <= targets.ends.astype(np.int64)[np.maximum(tgt, 0)])
            tid = tgt.astype(np.int64).astype(np.uint32) if len(tgt) else np.zeros(0, dtype=np.uint32)
        use = use.astype(np.uint8)
    return pair_chains(rec.rs, rec.re, t.rev, t.score, offs, tid, use, sel.mapq, **params)


MateRescue = collections.namedtuple("MateRescue", "read edits rs re rev span offsets ops")
RescueRequests = collections.namedtuple("RescueRequests", "q_lo q_hi w_lo w_hi rev read")
RESCUE_NONE, RESCUE_OVER = -1, -2                    # KH_RESCUE_NONE, KH_RESCUE_OVER in MateRescue.edits
RESCUE_MAX_READ, RESCUE_MAX_WINDOW = 512, 65536      # KH_RESCUE_MAX_READ, KH_RESCUE_MAX_WINDOW


def rescue_mates(qtext, rtext, q_lo, q_hi, w_lo, w_hi, rev, ref_base=0, max_edits=31, device=0):
    """mates without a row aligned end to end inside a window of the reference (kh_mate_rescue in include/kmerhash_amd.h, which holds the
    definition).  Request j: the mate qtext[q_lo[j]:q_hi[j]] (at most 512 bases), as it stands where bit 0 of rev[j] is clear and as its
    reverse complement where it is set, against the window [w_lo[j], w_hi[j]) of global reference coordinates (at most 65536 bases;
    rtext covers [ref_base, ref_base + len(rtext))).  The whole window is scanned for the end column of least edit distance d* (ties:
    the first), then the alignment is traced back from there; max_edits 0..31.
    -> MateRescue(read, edits, rs, re, rev, span, offsets, ops): read = the request's number (index.map_pairs_rescued puts the read
    number there); edits = d*, RESCUE_NONE (-1: a request outside the texts or the limits) or RESCUE_OVER (-2: d* > max_edits);
    [rs, re) the reference interval, rev as given, span = the distance from the first to the last end column attaining d* (more than
    d*: a second placement inside the window); then a CSR of runs (len << 4) | op in reference order (=, X, I, D; end to end, no S).
    Count, then emit: two calls, one allocation of the exact size.  numpy in, numpy out (uint32, int32, uint32 x 2, uint8, uint32,
    uint64, uint32); CUDA tensors in, tensors out on the current stream (int32 holding the uint32 bits, int64 offsets); the call waits
    for the stream once per pass.  At most 2^24 requests per call."""
    if not 0 <= int(max_edits) <= 31:
        raise ValueError("max_edits must be 0..31 (one diagonal per lane of a wavefront), got %r" % (max_edits,))
    tq, tr = _Buf.text(qtext), _Buf.text(rtext)
    lb, hb, wl, wh, vb = _Buf(q_lo, np.uint32), _Buf(q_hi, np.uint32), _Buf(w_lo, np.uint32), _Buf(w_hi, np.uint32), _Buf(rev, np.uint8)
    check_same("the texts, q_lo, q_hi, w_lo, w_hi and rev must live in the same memory", tq, tr, lb, hb, wl, wh, vb, length=False)
    n = lb.n
    check_same("q_lo, q_hi, w_lo, w_hi and rev must have one entry per request, got %d, %d, %d, %d and %d" % (n, hb.n, wl.n, wh.n, vb.n), lb, hb, wl, wh, vb)
    _check_text_limits(1, 0, tq, tr, ref_base)
    if n > 2 ** 24:
        raise ValueError("at most 2^24 requests per call (batch over reads), got %d" % n)
    edits, eptr = alloc(lb, n, np.int32, empty=True)
    nums = [alloc(lb, n, np.uint32, empty=True) for _ in range(3)]
    offs, optr = alloc(lb, n + 1, np.uint64, zero=True)
    read = torch.arange(n, dtype=torch.int32, device=lb.device) if lb.dev else np.arange(n, dtype=np.uint32)
    if n == 0:      # nothing to queue: the zeroed offset is the answer
        return MateRescue(read, edits, nums[0][0], nums[1][0], vb.obj, nums[2][0], offs, alloc(lb, 0, np.uint32)[0])
    args = (tq.ptr_or_null, tq.n, tr.ptr_or_null, tr.n, int(ref_base), lb.ptr, hb.ptr, wl.ptr, wh.ptr, vb.ptr, n, int(max_edits), lb.where, eptr,
            *(p for _, p in nums), optr)
    ops = two_pass("kh_mate_rescue", args, lb, np.uint32, device)
    return MateRescue(read, edits, nums[0][0], nums[1][0], vb.obj, nums[2][0], offs, ops)


def rescue_requests(mapping, pairs, read_starts, read_ends, min_ins=0, max_ins=1000, max_edits=31, targets=None, ref_len=None, ref_base=0):
    """the requests of rescue_mates for the mates pairing left without a row, derived with array operations where the Mapping lives (no
    column goes to the host; the one wait is the one that learns how many requests there are).  mapping, pairs: what index.map_pairs
    returned; read_starts / read_ends: the byte interval of every read in the query text -- CUDA tensors are used where they are, host
    arrays next to a device Mapping are uploaded.
    Mate Y of a pair gets a request iff pairs.row[Y] == -1, its partner X has a representative row pairs.row[X] >= 0, and that row lies
    on a target (with targets: targets.locate(rs) names one).  Only concordant places of a forward-reverse library are searched.  With
    m the length of Y and [rs, re) the interval of X's row:
      X forward: Y is expected reverse (rev = 1) in [max(rs, rs + min_ins - m - max_edits), rs + max_ins);
      X reverse: Y is expected forward (rev = 0) in [re - max_ins, min(re, re - min_ins + m + max_edits)).
    Both windows are clamped to X's target -- targets (a kmerhash_amd.Targets), or [ref_base, ref_base + ref_len) -- and to
    RESCUE_MAX_WINDOW bases, of which the ones nearest to X are kept.
    -> RescueRequests(q_lo, q_hi, w_lo, w_hi, rev, read): the arguments of rescue_mates and the read number of every request,
    ascending."""
    _check_pair_params(min_ins, max_ins, 0)
    if not 0 <= int(max_edits) <= 31:
        raise ValueError("max_edits must be 0..31, got %r" % (max_edits,))
    if targets is None and ref_len is None:
        raise ValueError("ref_len is needed without targets: the windows are clamped to [ref_base, ref_base + ref_len)")
    row, rec, trev = pairs.row, mapping.records, mapping.table.rev
    dev = _is_tensor(row) and row.is_cuda
    n_reads = int(row.numel() if dev else len(row))
    if n_reads % 2:
        raise ValueError("reads come in pairs (mate 1, mate 2, ...): an even number of reads is needed, got %d" % n_reads)

    def offsets(x):      # a column of byte offsets where the Mapping lives: a CUDA tensor stays on its device, anything else is uploaded once
        if dev and _is_tensor(x) and x.is_cuda:
            return x.long().ravel()
        a = np.asarray(x.cpu() if _is_tensor(x) else x, dtype=np.int64).ravel()
        return torch.from_numpy(a).to(row.device) if dev else a

    starts, ends = offsets(read_starts), offsets(read_ends)
    if len(starts) != n_reads or len(ends) != n_reads:
        raise ValueError("read_starts and read_ends must hold one entry per read of pairs (%d), got %d and %d" % (n_reads, len(starts), len(ends)))
    min_ins, max_ins, max_edits = int(min_ins), int(max_ins), int(max_edits)
    if dev:
        where, lo_, hi_ = torch.where, torch.maximum, torch.minimum
        i64 = lambda x, mask=False: (x.long() & 0xFFFFFFFF) if mask else x.long()      # noqa: E731
        idx = torch.arange(n_reads, dtype=torch.int64, device=row.device)
        const = lambda v: torch.full((n_reads,), int(v), dtype=torch.int64, device=row.device)      # noqa: E731
    else:
        where, lo_, hi_ = np.where, np.maximum, np.minimum
        i64 = lambda x, mask=False: np.asarray(x).astype(np.int64)      # noqa: E731
        idx = np.arange(n_reads, dtype=np.int64)
        const = lambda v: np.full(n_reads, int(v), dtype=np.int64)      # noqa: E731
        row, trev = _host(row, np.int32), _host(trev, np.uint8)
    own, n_rows = i64(row), int(rec.rs.numel() if dev else len(rec.rs))
    prow = own[idx ^ 1]
    need = (own == -1) & (prow >= 0) & (prow < n_rows)
    if n_rows == 0 or n_reads == 0:
        empty = [alloc(_Buf(row, np.int32), 0, dt)[0] for dt in (np.uint32, np.uint32, np.uint32, np.uint32, np.uint8, np.uint32)]
        return RescueRequests(*empty)
    at = where(need, prow, const(0))
    prs, pre = (i64(x if dev else _host(x, np.uint32), True)[at] for x in (rec.rs, rec.re))
    fwd = (i64(trev)[at] & 1) == 0
    if targets is not None:
        tgt, _ = targets.locate(prs)
        need = need & (tgt >= 0)
        tc = where(tgt >= 0, tgt, const(0))
        if dev:
            ts, te = (x.long() & 0xFFFFFFFF for x in targets.to(row.device))
        else:
            ts, te = targets.starts.astype(np.int64), targets.ends.astype(np.int64)
        tlo, thi = ts[tc], te[tc]
    else:
        tlo, thi = const(ref_base), const(int(ref_base) + int(ref_len))
    m = ends - starts
    w_lo = where(fwd, lo_(prs, prs + (min_ins - max_edits) - m), pre - max_ins)
    w_hi = where(fwd, prs + max_ins, hi_(pre, pre - (min_ins - max_edits) + m))
    w_lo = hi_(lo_(w_lo, tlo), thi)
    w_hi = lo_(hi_(w_hi, thi), w_lo)
    w_hi = where(fwd, hi_(w_hi, w_lo + RESCUE_MAX_WINDOW), w_hi)
    w_lo = where(fwd, w_lo, lo_(w_lo, w_hi - RESCUE_MAX_WINDOW))
    if dev:
        sel = torch.nonzero(need).ravel()      # (the one wait: the number of requests)
        return RescueRequests(starts[sel].int(), ends[sel].int(), w_lo[sel].int(), w_hi[sel].int(), fwd[sel].to(torch.uint8), sel.int())
    sel = np.flatnonzero(need)
    return RescueRequests(starts[sel].astype(np.uint32), ends[sel].astype(np.uint32), w_lo[sel].astype(np.uint32), w_hi[sel].astype(np.uint32),
                          fwd[sel].astype(np.uint8), sel.astype(np.uint32))


def read_cigar(cigars, ends, table, row, k):
    """the CIGAR of the whole read of chain `row` as text (a host helper like cigar_string): 'S' for the bases the head clips, the head's
    row, what cigar_string(cigars, table, row, k) gives, the tail's row, 'S' for the bases the tail clips, equal neighbours merged -- in
    read order, for a reverse-strand chain too; with extended_intervals() it is the alignment record of the read.  None where
    cigar_string is None."""
    mid = cigar_string(cigars, table, row, k)
    if mid is None:
        return None
    import re
    offs, ops, clip = _host(ends.offsets, np.int64), _host(ends.ops, np.uint32), _host(ends.clip, np.uint32)
    h, t = 2 * int(row), 2 * int(row) + 1
    runs = [("S", int(clip[h]))] + [(CIGAR_OPS[int(v) & 15], int(v) >> 4) for v in ops[offs[h]:offs[h + 1]]]
    runs += [(o, int(n)) for n, o in re.findall(r"(\d+)([ID=X])", mid)]
    runs += [(CIGAR_OPS[int(v) & 15], int(v) >> 4) for v in ops[offs[t]:offs[t + 1]]] + [("S", int(clip[t]))]
    out = []
    for op, n in runs:
        if n == 0:
            continue
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return "".join("%d%s" % (n, op) for op, n in out)


def extended_intervals(table, ends):
    """the intervals of a ChainTable with the ends added (a host helper) -> (q_start, q_end, r_start, r_end), int64 arrays with one entry
    per row: the head moves q_start down and the tail q_end up by the read bases they align; on the forward strand the head moves r_start
    down and the tail r_end up by the reference bases they face, on the reverse strand the head extends r_end and the tail r_start."""
    q0, q1, r0, r1 = (_host(x, np.uint32).astype(np.int64) for x in (table.q_start, table.q_end, table.r_start, table.r_end))
    rev = _host(table.rev, np.uint8).astype(bool)
    eq, er = _host(ends.q, np.uint32).astype(np.int64), _host(ends.r, np.uint32).astype(np.int64)
    hq, tq, hr, tr = eq[0::2], eq[1::2], er[0::2], er[1::2]
    return q0 - hq, q1 + tq, r0 - np.where(rev, tr, hr), r1 + np.where(rev, hr, tr)


ChainRecords = collections.namedtuple("ChainRecords", "valid qs qe rs re qlen n_match n_block nm offsets ops")
Mapping = collections.namedtuple("Mapping", "table edits cigars ends select records")
TEXT_OPS = "MIDNSHP=X"      # the op letters kh_cigar_text prints; '?' for the codes 9..15


def chain_records(qpos, rpos, rev, chain, cigars, first, last, q_lo, q_hi, ends, k, ref_order=False, device=0):
    """one alignment record per chain (kh_chain_records in include/kmerhash_amd.h, which holds the definition), from what the chain calls
    wrote and nothing else: the anchors with their chain numbers, the ChainCigars of chain_cigars, first / last / q_lo / q_hi as
    chain_ends took them and the ChainEnds it returned.
    -> ChainRecords(valid, qs, qe, rs, re, qlen, n_match, n_block, nm, offsets, ops): per chain whether it has a whole alignment, the
    read-relative query interval, the reference interval, the read's length, the matching bases, the alignment block length and the
    edits (PAF columns 3, 4, 8, 9, 2, 10, 11 and NM); then a CSR whose row c is the CIGAR of the whole read of chain c as runs
    (len << 4) | op -- S, the head, the links, k '=', the tail, S, equal neighbours merged: what read_cigar() prints.  ref_order: the
    rows of reverse-strand chains are stored back to front, as PAF and SAM want them.  An invalid chain has an empty row.  Count, then
    emit: two calls, one allocation of the exact size.  numpy in, numpy out (uint8, uint32 x 8, uint64, uint32); CUDA tensors in, tensors
    out on the current stream (int32 holding the uint32 bits, int64 offsets); the call waits for the stream once per pass.  At most 2^24
    anchors and 2^23 chains per call.  cigar_text() renders the rows, write_paf() the lines."""
    if not 1 <= int(k) <= 64:
        raise ValueError("k must be 1..64, got %r" % (k,))
    qb, rb, vb, cb = _Buf(qpos, np.uint32), _Buf(rpos, np.uint32), _Buf(rev, np.uint8), _Buf(chain, np.int32)
    lo_, lp = _Buf(cigars.offsets, np.uint64), _Buf(cigars.ops, np.uint32)
    fb, lb, ob, hb = _Buf(first, np.uint32), _Buf(last, np.uint32), _Buf(q_lo, np.uint32), _Buf(q_hi, np.uint32)
    eq, er, ec, eo, ep = _Buf(ends.q, np.uint32), _Buf(ends.r, np.uint32), _Buf(ends.clip, np.uint32), _Buf(ends.offsets, np.uint64), _Buf(ends.ops, np.uint32)
    check_same("the anchors, the cigars, first, last, q_lo, q_hi and the ends must live in the same memory", qb, rb, vb, cb, lo_, lp, fb, lb, ob, hb, eq, er, ec, eo, ep,
               length=False)
    m, nc = qb.n, fb.n
    check_same("qpos, rpos, rev and chain must have one entry per anchor, got %d, %d, %d and %d" % (m, rb.n, vb.n, cb.n), qb, rb, vb, cb)
    check_same("first, last, q_lo and q_hi must have one entry per chain, got %d, %d, %d and %d" % (nc, lb.n, ob.n, hb.n), fb, lb, ob, hb)
    if lo_.n != m + 1:
        raise ValueError("cigars.offsets must hold one entry per anchor and one more, got %d for %d anchors" % (lo_.n, m))
    if eq.n != 2 * nc or er.n != 2 * nc or ec.n != 2 * nc or eo.n != 2 * nc + 1:
        raise ValueError("the ends must hold two rows per chain (q, r, clip: %d, %d, %d; offsets: %d) for %d chains" % (eq.n, er.n, ec.n, eo.n, nc))
    if m > 2 ** 24:
        raise ValueError("at most 2^24 anchors per call (batch over reads), got %d" % m)
    if nc > 2 ** 23:
        raise ValueError("at most 2^23 chains per call (batch over reads), got %d" % nc)
    valid, vptr = alloc(fb, nc, np.uint8, empty=True)
    nums = [alloc(fb, nc, np.uint32, empty=True) for _ in range(8)]
    offs, optr = alloc(fb, nc + 1, np.uint64, zero=True)
    if nc == 0:      # nothing to queue: the zeroed offset is the answer
        return ChainRecords(valid, *(a for a, _ in nums), offs, alloc(fb, 0, np.uint32)[0])
    args = (qb.ptr_or_null, rb.ptr_or_null, vb.ptr_or_null, cb.ptr_or_null, m, lo_.ptr if m else None, lp.ptr_or_null, lp.n, fb.ptr, lb.ptr, ob.ptr, hb.ptr, nc,
            eq.ptr, er.ptr, ec.ptr, eo.ptr, ep.ptr_or_null, ep.n, int(k), 1 if ref_order else 0, fb.where, vptr, *(p for _, p in nums), optr)
    return ChainRecords(valid, *(a for a, _ in nums), offs, two_pass("kh_chain_records", args, fb, np.uint32, device))


def cigar_text(offsets, ops, device=0):
    """a CSR of runs (len << 4) | op as CIGAR text (kh_cigar_text): row i becomes the decimal length and the op letter ("MIDNSHP=X", '?'
    beyond) of each of its runs.  Any run CSR will do: ChainCigars, ChainEnds or ChainRecords offsets / ops.
    -> (text_offsets, text): row i is text[text_offsets[i]:text_offsets[i + 1]].  numpy in (uint64, uint32), numpy out (uint64, uint8);
    CUDA tensors in (int64, int32), tensors out (int64, uint8) on the current stream; count, then emit, one wait per pass."""
    ob, pb = _Buf(offsets, np.uint64), _Buf(ops, np.uint32)
    check_same("offsets and ops must live in the same memory", ob, pb, length=False)
    if ob.n < 1:
        raise ValueError("offsets must hold n_rows + 1 >= 1 entries")
    rows = ob.n - 1
    if rows > 2 ** 31 or pb.n > 2 ** 31:
        raise ValueError("at most 2^31 rows and 2^31 runs per call, got %d and %d" % (rows, pb.n))
    toff, tptr = alloc(ob, rows + 1, np.uint64, zero=True)
    if rows == 0 or pb.n == 0:      # nothing to queue: the zeroed offsets are the answer
        return toff, alloc(ob, 0, np.uint8)[0]
    return toff, two_pass("kh_cigar_text", (ob.ptr, rows, pb.ptr, pb.n, ob.where, tptr), ob, np.uint8, device)


def paf_lines(mapping, text_offsets, text, read_names, ref_name=None, ref_len=None, k=None, ref_start=0, kept_only=True, targets=None, cs=None):
    """the formatting half of write_paf() (host only): the columns of a Mapping and the text CSR of its record rows -> (lines, skipped).
    cs: a RecordDiffs of kind "cs" over the mapping's records (sam.record_diffs), printed as a trailing cs:Z: tag"""
    if targets is not None:
        if ref_name is not None or ref_len is not None or int(ref_start) != 0:
            raise ValueError("with targets the names, lengths and starts are theirs: ref_name and ref_len must be None and ref_start 0")
    elif ref_name is None or ref_len is None:
        raise ValueError("ref_name and ref_len are needed without targets")
    t, sel, rec = mapping.table, mapping.select, mapping.records
    seg, rev, count, score = _host(t.seg, np.uint32), _host(t.rev, np.uint8), _host(t.count, np.uint32), _host(t.score, np.int32)
    flag, mapq, sub = _host(sel.flag, np.uint8), _host(sel.mapq, np.uint8), _host(sel.sub, np.int32)
    valid = _host(rec.valid, np.uint8)
    cols = [_host(x, np.uint32) for x in (rec.qlen, rec.qs, rec.qe, rec.rs, rec.re, rec.n_match, rec.n_block, rec.nm)]
    toff, raw = _host(text_offsets, np.int64), _host(text, np.uint8).tobytes().decode("ascii")
    if cs is not None:
        cs_off, cs_raw = _host(cs.offsets, np.int64), _host(cs.text, np.uint8).tobytes().decode("ascii")
    if targets is not None:      # a row's target is the one its first reference base lies in; its end must lie there too
        tgt, local = targets.locate(cols[3])
        inside = (tgt >= 0) & (cols[4].astype(np.int64) <= targets.ends.astype(np.int64)[np.maximum(tgt, 0)])
    lines, skipped = [], 0
    for c in range(len(valid)):
        if kept_only and not flag[c] & FLAG_KEPT:
            continue
        if not valid[c] or (targets is not None and not inside[c]):
            skipped += 1
            continue
        qlen, qs, qe, rs, re_, n_match, n_block, nm = (int(x[c]) for x in cols)
        pri = bool(flag[c] & FLAG_PRIMARY)
        if targets is None:
            tname, tlen, t0 = str(ref_name), int(ref_len), int(ref_start)
        else:
            tname, tlen, t0 = targets.names[int(tgt[c])], int(targets.lengths[int(tgt[c])]), int(targets.starts[int(tgt[c])])
        f = [str(read_names[int(seg[c])]), qlen, qs, qe, "-" if rev[c] & 1 else "+", tname, tlen, rs - t0, re_ - t0, n_match, n_block,
             int(mapq[c]), "tp:A:%s" % ("P" if pri else "S"), "cm:i:%d" % int(count[c]), "s1:i:%d" % int(score[c])]
        if pri:
            f.append("s2:i:%d" % int(sub[c]))
        f += ["NM:i:%d" % nm, "cg:Z:%s" % raw[toff[c]:toff[c + 1]]]
        if cs is not None:
            f.append("cs:Z:%s" % cs_raw[cs_off[c]:cs_off[c + 1]])
        lines.append("\t".join(str(x) for x in f))
    return lines, skipped


def write_paf(fh, mapping, read_names, ref_name=None, ref_len=None, k=None, ref_start=0, kept_only=True, device=0, targets=None, cs=None):
    """the rows of a Mapping (index.map) as PAF lines into the text file `fh`: one cigar_text() call over the records, one copy of every
    column to the host, then one line per row -- qname qlen qs qe strand tname tlen rs-ref_start re-ref_start n_match n_block mapq,
    then tp:A:P|S, cm:i:<anchors>, s1:i:<chain score>, s2:i:<best secondary score> (primaries only), NM:i:<edits>, cg:Z:<CIGAR>.
    read_names[s]: the name of read s; one target (ref_name, ref_len) whose base 0 is reference coordinate ref_start.  kept_only: only
    the rows select kept (flag bit 1).  Rows without a whole alignment (valid == 0) are skipped.  Make the Mapping with ref_order=True:
    PAF wants the CIGAR of a reverse-strand row in reference order.  targets: the kmerhash_amd.Targets the Mapping was made with
    (index.map(..., targets=T)) -- columns 6 to 9 are then the row's own target name, its length and the target-local interval, and
    ref_name / ref_len / ref_start stay None / None / 0; a row whose interval does not lie inside one target counts as skipped.
    cs: a RecordDiffs of kind "cs" for the mapping's records (sam.record_diffs) -- every line then ends with cs:Z:<text>, what
    paftools call reads; None: no such tag.
    -> (lines written, rows skipped as invalid)"""
    toff, text = cigar_text(mapping.records.offsets, mapping.records.ops, device)
    lines, skipped = paf_lines(mapping, toff, text, read_names, ref_name, ref_len, k, ref_start, kept_only, targets, cs)
    for ln in lines:
        fh.write(ln + "\n")
    return len(lines), skipped


class KmerCounter:
    """counting index: k-mer -> number of occurrences (Reducer = std::plus, value 1 per occurrence)"""

    def __init__(self, k=31, canonical=True, hash="farm", min_load_factor=0.35, max_load_factor=0.8, device=0, reserve_from_estimate=False):
        """reserve_from_estimate: size the table before every insert from a HyperLogLog estimate of the distinct k-mers seen so far
        (the reference's counting table does, robinhood_offset_hashmap_ptr.hpp:2484-2535): the batch text first goes through the fused
        text -> registers pass (no k-mer buffer), the estimator accumulates over the batches.  Every k in 1..64."""
        self.k, self.canonical, self.device = k, canonical, device
        # 33 <= k <= 64: 16-byte k-mers in the wide table (k-mer = {w0, w1}, see kmerhash_amd.wide)
        self.wide = 32 < k <= 64
        cls = hashmap_robinhood_doubling_wide if self.wide else hashmap_robinhood_doubling
        self.table = cls(128, min_load_factor, max_load_factor, hash=hash, seed=43, device=device)
        self.reserve_from_estimate = reserve_from_estimate
        self._hash, self.hll = hash, None

    def _presize(self, text, fastq):
        if self.hll is None:      # the table's hash, seed 43, precision 12 (the reference's hyperloglog64<Key, Hash, 12>)
            self.hll = hyperloglog64(12, 0, self._hash, 43, self.device)
        (self.hll.update_from_fastq if fastq else self.hll.update_from_sequence)(text, self.k, self.canonical)
        est = self.hll.estimate()
        self.table.reserve(int(est * (1.0 + self.hll.est_error_rate)))
        return est

    def presize_sequences(self, seq):
        """the estimate and reserve steps of add_sequences alone: feeds the counter's estimator with the k-mers of `seq` (fused pass)
        and reserves the table for the estimated number of distinct k-mers (+ the estimator's standard error); returns the estimate"""
        return self._presize(seq, False)

    def presize_fastq(self, text):
        """presize_sequences over raw FASTQ text"""
        return self._presize(text, True)

    def _kmers(self, seq, fastq):
        if self.wide:
            return kmers128_from_sequence(seq, self.k, self.canonical, self.device, _fastq=fastq)
        return kmers_from_sequence(seq, self.k, self.canonical, self.device, _fastq=fastq)

    def add_sequences(self, seq):
        if self.reserve_from_estimate:
            self._presize(seq, False)
        km = self._kmers(seq, False)
        if len(km):
            self.table.insert_reduce_plus(km)
        return len(km)

    def add_fastq(self, buf):
        """raw FASTQ text (whole records), host or device: record structure, k-mer generation and counting all run on the GPU"""
        if self.reserve_from_estimate:
            self._presize(buf, True)
        km = self._kmers(buf, True)
        if len(km):
            self.table.insert_reduce_plus(km)
        return len(km)

    def counts(self, min_count=0):
        """(k-mers, counts) in slot order; min_count > 0: only the k-mers that occur at least that often (selected on the GPU)"""
        if min_count <= 0:
            return self.table.to_vector()
        return self.table.select_values(min(int(min_count), 0xFFFFFFFF), 0xFFFFFFFF)

    def spectrum(self, nbins=256):
        """the k-mer spectrum: uint64[nbins], entry c = number of distinct k-mers that occur c times, the last entry those that
        occur nbins - 1 times or more (entry 0 stays 0: a stored k-mer occurs at least once)"""
        return self.table.value_histogram(nbins)

    def drop_below(self, min_count):
        """abundance filter: erases the k-mers that occur fewer than min_count times (sequencing errors); returns their number"""
        if min_count <= 0:
            return 0
        return self.table.erase_values(0, min(int(min_count), 1 << 32) - 1)

    def write(self, filename, count_dtype=np.uint16):
        """raw (k-mer, count) tuples, sizeof(KmerType) + sizeof(CountType) bytes each, no padding
        (BenchmarkKmerCounter.cpp:1022-1059 copyToByteArray; CountType = uint16_t there, wrapping like std::plus)"""
        k, v = self.counts()
        # (k > 32: the 16-byte k-mer {w0, w1}, sizeof(Kmer<63, DNA, uint64_t>) + sizeof(CountType) per tuple)
        kt = np.dtype(("<u8", (2,))) if self.wide else np.dtype("<u8")
        rec = np.zeros(len(k), dtype=np.dtype([("kmer", kt), ("count", np.dtype(count_dtype).newbyteorder("<"))]))
        rec["kmer"] = k
        rec["count"] = v.astype(count_dtype)
        rec.tofile(filename)
        return len(k)

    def close(self):
        self.table.close()
        if self.hll is not None:
            self.hll.close()


def synthetic_fastq(n_reads, read_len=150, genome_len=1_000_000, seed=7, n_rate=0.001):
    """random genome, uniformly sampled reads on both strands, a sprinkle of N's (SURVEY §8d W5 shape, scaled)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len, dtype=np.uint8)
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    starts = rng.integers(0, genome_len - read_len, n_reads)
    rev = rng.integers(0, 2, n_reads).astype(bool)
    out = []
    for i in range(n_reads):
        r = genome[starts[i]: starts[i] + read_len]
        if rev[i]:
            r = comp[r[::-1]]
        s = lut[r].copy()
        m = rng.random(read_len) < n_rate
        s[m] = ord("N")
        out.append(b"@r%d\n" % i + s.tobytes() + b"\n+\n" + b"I" * read_len + b"\n")
    return b"".join(out)


def synthetic_read_sequences(n_reads, read_len=150, genome_len=1_000_000, seed=7, n_rate=0.001):
    """the sequence lines of synthetic_fastq's reads without the FASTQ text around them (vectorised: for large inputs):
    uint8 array of n_reads lines of read_len bases, each followed by a newline"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len, dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = np.empty((n_reads, read_len + 1), dtype=np.uint8)
    ar = np.arange(read_len, dtype=np.int32)[None, :]
    for c0 in range(0, n_reads, 100_000):                      # chunked: the index matrix stays cache/L2 sized
        c1 = min(n_reads, c0 + 100_000)
        starts = rng.integers(0, genome_len - read_len, c1 - c0, dtype=np.int32)
        rev = rng.integers(0, 2, c1 - c0, dtype=np.uint8).astype(bool)
        r = genome[starts[:, None] + ar]
        r[rev] = (3 - r[rev])[:, ::-1]
        blk = out[c0:c1, :read_len]
        blk[...] = lut[r]
        n_n = rng.binomial((c1 - c0) * read_len, n_rate)
        if n_n:
            blk[rng.integers(0, c1 - c0, n_n), rng.integers(0, read_len, n_n)] = ord("N")
    out[:, read_len] = 10
    return out.reshape(-1)


def synthetic_fastq_fixed(n_reads, read_len=150, genome_len=1_000_000, seed=7, n_rate=0.001):
    """raw FASTQ text of synthetic_read_sequences' reads (vectorised, fixed-width records: '@' + 11-digit id, sequence, '+',
    quality 'I' * read_len), as a uint8 array -- the input shape of BenchmarkKmerCounter, for the GPU FASTQ path"""
    return fastq_from_sequence_lines(synthetic_read_sequences(n_reads, read_len, genome_len, seed, n_rate), n_reads, read_len)


class ShardedKmerCounter:
    """BASELINE configs[4]: the distributed k-mer counter.  BenchmarkKmerCounter.cpp:1476-1787 reads the input in file batches,
    turns every batch into canonical k-mers, and inserts them into dsc::counting_batched_robinhood_map (Reducer = std::plus,
    distributed_batched_robinhood_map.hpp:2542-2950): every rank parses ITS share of the reads, the k-mers are sharded by
    murmur3(k-mer, seed 9876543) over the ranks (kmerhash_amd.dist.ShardedTable: RCCL exchange, pipelined) and counted in the
    owner's local table, which starts at capacity 128 and doubles under load (or is pre-sized from a HyperLogLog estimate,
    robinhood_offset_hashmap_ptr.hpp:2512-2535, with reserve_from_estimate=True).  cycle() is the query phase of
    BenchmarkKmerIndex.cpp:787-843: count, find, erase over a sample of the input, then count again.

    `sharded` is a kmerhash_amd.dist.ShardedTable (any backend); `kmer_fn(text) -> packed canonical k-mers` is the k-mer
    generator (default: kh_kmers_from_fastq on this rank's GPU; kh_kmers128_from_fastq when 32 < k <= 64, which needs a backend
    of 16-byte keys such as kmerhash_amd.dist.WideGpuBackend).  `hll`: the estimator of reserve_from_estimate (anything with
    update / update_wide, registers(), precision and est_error_rate; update_wide takes the (n, 2) k-mers of k > 32).
    estimate_from_text: the estimator is fed from the batch TEXT by the fused pass (hll.update_from_fastq(text, k, canonical): no
    k-mer is read back) instead of from the generated k-mers; the all-reduce(max) of the registers and the per-rank share are the same.
    Raises ValueError up front for k outside 1..64, for a sharded table whose key width does not match k, for
    reserve_from_estimate with k > 32 and no hll (the HyperLogLog must then be one with update_wide), and for estimate_from_text
    without reserve_from_estimate and an hll that has update_from_fastq."""

    def __init__(self, sharded, k=31, canonical=True, kmer_fn=None, chunks=1, reserve_from_estimate=False, hll=None,
                 estimate_from_text=False):
        if not 1 <= k <= 64:
            raise ValueError("k must be 1..64, got %d" % k)
        # 33 <= k <= 64: 16-byte k-mers {w0, w1}, an (n, 2) tensor per batch, over a backend with key_words = 2
        self.wide = k > 32
        words = int(getattr(sharded.b, "key_words", 1))
        if words != (2 if self.wide else 1):
            raise ValueError("k = %d needs a sharded table of %d-byte keys, this one holds %d-byte keys (backend key_words = %d)"
                             % (k, 16 if self.wide else 8, 8 * words, words))
        if self.wide and reserve_from_estimate and (hll is None or not hasattr(hll, "update_wide")):
            raise ValueError("reserve_from_estimate with k > 32 needs hll=: a HyperLogLog with update_wide (16-byte keys)")
        if estimate_from_text and not (reserve_from_estimate and hasattr(hll, "update_from_fastq")):
            raise ValueError("estimate_from_text needs reserve_from_estimate and hll=: a HyperLogLog with update_from_fastq")
        self.estimate_from_text = estimate_from_text
        self.st, self.k, self.canonical, self.chunks = sharded, k, canonical, chunks
        dev = getattr(sharded.b, "device", 0)
        default_fn = kmers128_from_fastq if self.wide else kmers_from_fastq
        self.kmer_fn = kmer_fn if kmer_fn is not None else (lambda text: default_fn(text, k, canonical, dev))
        self.reserve_from_estimate = reserve_from_estimate
        self.hll = hll
        self.total_kmers = 0

    def add_fastq(self, text):
        """one file batch of this rank: raw FASTQ text (whole records) -> k-mers -> sharded counting insert.  Collective: every
        rank calls it once per batch (an empty batch where a rank has run out of reads)."""
        km = self.kmer_fn(text)
        if self.reserve_from_estimate and self.hll is not None:
            # the reference sizes its counting table from a HyperLogLog estimate of the distinct k-mers seen so far (+ the
            # estimator's standard error 1.04 / sqrt(m)) before it inserts: every rank updates its registers with ITS k-mers, the
            # registers are merged over all ranks (all-reduce(max): hyperloglog64.hpp:477-484 merge_distributed / estimate_global) and
            # every rank reserves its share of the global estimate (estimate_average_per_rank :487-489).  Collective: all ranks, every batch.
            if self.estimate_from_text:
                if len(text):
                    self.hll.update_from_fastq(text, self.k, self.canonical)
            elif len(km):
                (self.hll.update_wide if self.wide else self.hll.update)(km)
            est = estimate_average_per_rank(self.hll, self.st.group)
            self.st.local.reserve(int(est * (1.0 + self.hll.est_error_rate)))
        self.st.insert_counts(km, chunks=self.chunks)
        self.total_kmers += len(km)
        return len(km)

    def cycle(self, queries):
        """count -> find -> erase -> count over `queries` (this rank's sample; collective).  Returns per-rank numbers:
        hits of the first count, sum of the counts find returned, keys erased on this rank's local table, hits afterwards."""
        cuda = getattr(queries, "is_cuda", False)

        def lap(t0):
            if cuda:
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        ms = {}
        t0 = time.perf_counter(); _, c1 = self.st.count(queries); ms["count"] = lap(t0)
        t0 = time.perf_counter(); _, vals, found = self.st.find(queries); ms["find"] = lap(t0)
        t0 = time.perf_counter(); erased = self.st.erase(queries); ms["erase"] = lap(t0)
        t0 = time.perf_counter(); _, c2 = self.st.count(queries); ms["count2"] = lap(t0)
        if hasattr(self.st, "synchronize"):
            self.st.synchronize()
        occ = (vals.to(torch.int64) & 0xFFFFFFFF) * found.to(torch.int64)
        return {"count_hits": int(c1.sum()), "find_hits": int(found.sum()), "find_occurrences": int(occ.sum()),
                "erased_local": int(erased), "count_hits_after": int(c2.sum()), "phase_ms": {k: round(v, 3) for k, v in ms.items()}}

    def size(self):
        return self.st.size()

    def spectrum(self, nbins=256):
        """the k-mer spectrum over all ranks (collective: every rank calls it and receives the same uint64[nbins])"""
        return self.st.value_histogram(nbins)

    def drop_below(self, min_count):
        """abundance filter on this rank's local table (no exchange: a k-mer's count lives on its owner rank alone); returns the
        number of k-mers this rank erased"""
        if min_count <= 0:
            return 0
        return self.st.erase_values(0, min(int(min_count), 1 << 32) - 1)


def read_positions(n_reads, read_len, genome_len, read_seed):
    """(starts, strand flags) of the reads synthetic_reads draws for `read_seed`"""
    rng = np.random.default_rng(read_seed)
    starts = rng.integers(0, genome_len - read_len, n_reads, dtype=np.int32)
    rev = rng.integers(0, 2, n_reads, dtype=np.uint8).astype(bool)
    return starts, rev


def synthetic_reads(n_reads, read_len=150, genome_len=1_000_000, genome_seed=7, read_seed=8):
    """error-free reads of a random genome on both strands, with what is needed to PREDICT every k-mer's count: returns
    (sequence lines as synthetic_read_sequences lays them out, genome codes, read starts, strand flags).  Ranks of a
    distributed run share genome_seed and differ in read_seed."""
    genome = np.random.default_rng(genome_seed).integers(0, 4, genome_len, dtype=np.uint8)
    starts, rev = read_positions(n_reads, read_len, genome_len, read_seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = np.empty((n_reads, read_len + 1), dtype=np.uint8)
    ar = np.arange(read_len, dtype=np.int32)[None, :]
    for c0 in range(0, n_reads, 100_000):
        c1 = min(n_reads, c0 + 100_000)
        r = genome[starts[c0:c1, None] + ar]
        rr = rev[c0:c1]
        r[rr] = (3 - r[rr])[:, ::-1]
        out[c0:c1, :read_len] = lut[r]
    out[:, read_len] = 10
    return out.reshape(-1), genome, starts, rev


def fastq_from_sequence_lines(seq_lines, n_reads, read_len):
    """fixed-width FASTQ text around the given sequence lines: '@' + 11-digit id, the line, '+', quality 'I' * read_len per record"""
    seq = seq_lines.reshape(n_reads, read_len + 1)
    w = 1 + 11 + 1 + (read_len + 1) + 2 + (read_len + 1)
    out = np.empty((n_reads, w), dtype=np.uint8)
    out[:, 0] = ord("@")
    ids = np.arange(n_reads, dtype=np.int64)
    for d in range(11):
        out[:, 11 - d] = ord("0") + (ids % 10)
        ids //= 10
    out[:, 12] = 10
    out[:, 13: 13 + read_len + 1] = seq
    o = 13 + read_len + 1
    out[:, o] = ord("+"); out[:, o + 1] = 10
    out[:, o + 2: o + 2 + read_len] = ord("I")
    out[:, o + 2 + read_len] = 10
    return out.reshape(-1)


def expected_kmer_coverage(genome_len, starts, read_len, k):
    """cov[p] = number of reads that contain the k-mer starting at genome position p (either strand: the canonical k-mer of a
    window is the same on both): the count the table must hold for that k-mer when the genome's k-mers are all distinct"""
    d = np.zeros(genome_len + 1, dtype=np.int64)
    np.add.at(d, starts, 1)
    np.add.at(d, starts + (read_len - k + 1), -1)
    return np.cumsum(d)[:genome_len]


def canonical_kmers_at(genome, positions, k):
    """packed canonical k-mers of the genome windows starting at `positions` (numpy; A0 C1 G2 T3, first base most significant)"""
    pos = np.asarray(positions, dtype=np.int64)
    fw = np.zeros(len(pos), dtype=np.uint64)
    rc = np.zeros(len(pos), dtype=np.uint64)
    for j in range(k):
        c = genome[pos + j].astype(np.uint64)
        fw = (fw << np.uint64(2)) | c
        rc |= (np.uint64(3) - c) << np.uint64(2 * j)
    return np.minimum(fw, rc)


def synthetic_fastq_device(n_reads, read_len, genome_len, genome_seed, read_seed, device, chunk=1_000_000):
    """the reads of synthetic_reads / fastq_from_sequence_lines generated ON THE GPU (torch): for inputs of BenchmarkKmerCounter's
    size (configs[4]: 6.25 Gbp per rank = 4.2e7 reads, 13 GB of FASTQ text) host generation would take minutes.  Returns
    (fastq text: uint8 CUDA tensor of n_reads fixed-width records, genome codes: uint8 CUDA tensor, read starts: int64 CUDA tensor).
    The generator is torch's (not numpy's): the reads differ from synthetic_reads', the prediction of every count from the read
    positions works the same way."""
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev); g.manual_seed(genome_seed)
    genome = torch.randint(0, 4, (genome_len,), dtype=torch.uint8, device=dev, generator=g)
    g.manual_seed(read_seed)
    starts = torch.randint(0, genome_len - read_len, (n_reads,), dtype=torch.int64, device=dev, generator=g)
    rev = torch.randint(0, 2, (n_reads,), dtype=torch.uint8, device=dev, generator=g).bool()
    w = 1 + 11 + 1 + (read_len + 1) + 2 + (read_len + 1)
    out = torch.empty((n_reads, w), dtype=torch.uint8, device=dev)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    ar = torch.arange(read_len, dtype=torch.int64, device=dev)[None, :]
    o = 13 + read_len + 1
    for c0 in range(0, n_reads, chunk):
        c1 = min(n_reads, c0 + chunk)
        blk = out[c0:c1]
        blk[:, 0] = ord("@")
        ids = torch.arange(c0, c1, dtype=torch.int64, device=dev)
        for d in range(11):
            blk[:, 11 - d] = (ord("0") + (ids % 10)).to(torch.uint8)
            ids = ids // 10
        blk[:, 12] = 10
        r = genome[starts[c0:c1, None] + ar]
        rr = rev[c0:c1]
        r[rr] = (3 - r[rr]).flip(1)
        blk[:, 13:13 + read_len] = lut[r.long()]
        blk[:, 13 + read_len] = 10
        blk[:, o] = ord("+"); blk[:, o + 1] = 10
        blk[:, o + 2:o + 2 + read_len] = ord("I")
        blk[:, o + 2 + read_len] = 10
        del r
    return out.reshape(-1), genome, starts
