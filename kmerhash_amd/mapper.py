"""The read mapper on a stranded position index: anchors -> chains -> edits -> CIGARs -> ends -> selection -> records -> pairs -> mate
rescue -> PAF (kmerhash_amd.sam writes SAM).  Three layers, top to bottom of this file:

  the stage wrappers  one Python call per C entry point of include/kmerhash_amd.h (stamp_strand ... rescue_mates, chain_records,
                      cigar_text), with the namedtuples they return and the constants of the header;
  the glue steps      what turns one stage's columns into the next stage's arguments -- the read layout, the segments of reads, the
                      ChainTable rows, the per-chain read intervals, the seg -> offsets CSR, the printable-row rule, the pair candidates,
                      the rescue windows -- each written once over an array namespace (kmerhash_amd._xp: numpy, or torch on a device);
  the pipeline        chains ... map_pairs_rescued as plain functions of an index, and map_fastq / map_fastq_pairs, which read a FASTQ
                      text (kmerhash_amd.fastq.read_fastq) and call them; the methods of KmerPositionIndex delegate here.

kmerhash_amd.kmers re-exports the public names under the module they were first published in."""
import collections
import ctypes as C

import numpy as np

from . import _capi as K
from ._call import _Buf, _is_tensor, alloc, check, check_same, stream_of, torch, two_pass
from ._xp import NUMPY, namespace_of
from .fastq import read_fastq
from .targets import Targets, inside_target


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


_host = NUMPY.col      # (column, dtype) -> the host array of its bits: what the host helpers below and the line formatters read


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
    rows = len(seg)
    if n_reads is None:
        n_reads = int(seg.max()) + 1 if rows else 0
    n_reads = int(n_reads)
    if n_reads < 0 or (rows and n_reads == 0):
        raise ValueError("n_reads must cover the reads of the table, got %r" % (n_reads,))
    if n_reads == 0:               # an empty table of no reads: nothing to select, no group to report
        _check_select_params(params.get("mask_pct", 50), params.get("pri_pct", 80), params.get("best_n", 5))
        like = _Buf(table.score, np.int32)
        return ChainSelect(*(alloc(like, 0, dt)[0] for dt in (np.int32, np.uint32, np.uint8, np.uint8, np.int32, np.uint32, np.int32)))
    offs = seg_offsets(namespace_of(seg), seg, n_reads, checked=True)      # (the check reads offs[-1]: on the device the one wait of this call)
    # select_chains is looked up where it is published: kmerhash_amd.kmers.select_chains replaced by a caller (another selection, a
    # stand-in) is what select_table calls, as it was while both lived in that module
    from . import kmers
    return kmers.select_chains(table.q_start, table.q_end, table.score, table.count, offs, **params)


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
    offs, use, tid = pair_candidates(namespace_of(t.seg), mapping, n_reads, targets)
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
    return rescue_windows(namespace_of(pairs.row), mapping, pairs, ReadLayout(read_starts, read_ends, None, 2), int(min_ins), int(max_ins), int(max_edits), targets, ref_len,
                          ref_base)


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
    cols = [_host(x, np.uint32) for x in (rec.qlen, rec.qs, rec.qe, rec.rs, rec.re, rec.n_match, rec.n_block, rec.nm)]
    toff, raw = _host(text_offsets, np.int64), _host(text, np.uint8).tobytes().decode("ascii")
    if cs is not None:
        cs_off, cs_raw = _host(cs.offsets, np.int64), _host(cs.text, np.uint8).tobytes().decode("ascii")
    good, considered, tgt = printable(NUMPY, mapping, targets, kept_only)
    lines, skipped = [], 0
    for c in np.flatnonzero(considered):
        if not good[c]:
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




# ---- the glue steps: each written once, over an array namespace xp (kmerhash_amd._xp) ------------------------------------------------
ChainTable = collections.namedtuple("ChainTable", "seg rev q_start q_end r_start r_end count score anchors chain")


class ReadLayout:
    """the byte interval [starts[s], ends[s]) of every read in a query text of n_text bytes, as the entry points take it: read_starts
    (None: one read, from byte 0) and read_ends (None: the next read's start, n_text for the last read).  Nothing is copied or checked
    before it is asked for: an entry point applies the checks it always applied, where it applied them."""

    def __init__(self, read_starts, read_ends, n_text, required=0):
        """required: how many of the two columns the entry point cannot default (the SAM writers: 1, rescue_requests: 2)"""
        if any(x is None for x in (read_starts, read_ends)[:required]):
            raise TypeError("read_starts%s must be given" % (" and read_ends" if required == 2 else ""))
        self.read_starts, self.read_ends, self.n_text, self._host = read_starts, read_ends, n_text, None

    @classmethod
    def of(cls, seq, read_starts, read_ends=None):
        """the layout of the reads in the text seq (a layout passed as read_starts is the answer: map_pairs_rescued makes one for all stages)"""
        return read_starts if isinstance(read_starts, cls) else cls(read_starts, read_ends, _Buf.text(seq).n)

    @property
    def n_reads(self):
        return 1 if self.read_starts is None else len(self.read_starts)

    @property
    def host(self):
        """(starts, ends) as int64 host arrays; a tensor is copied to the host, once"""
        if self._host is None:
            h = lambda x: np.asarray(x.cpu() if _is_tensor(x) else x, dtype=np.int64).ravel()      # noqa: E731
            rs = np.zeros(1, dtype=np.int64) if self.read_starts is None else h(self.read_starts)
            self._host = rs, (np.concatenate([rs[1:], [self.n_text]]) if self.read_ends is None else h(self.read_ends))
        return self._host

    def ascending(self):
        """the check of the chaining calls: the reads tile the text from byte 0"""
        rs = self.host[0]
        if rs.size == 0 or rs[0] != 0 or (np.diff(rs) < 0).any():
            raise ValueError("read_starts must be ascending byte offsets of the reads in seq, the first one 0")

    def bounded(self, every):
        """one end per read and read_starts[s] <= read_ends[s] <= len(seq).  every=False: the check of chain_ends and map, of read_ends
        that are given only; every=True: that of the SAM writers, of the default ends and of 0 <= read_starts[s] too"""
        rs, re_ = self.host
        if (every or self.read_ends is not None) and (re_.size != rs.size or (re_ < rs).any() or (re_ > self.n_text).any() or (every and (rs < 0).any())):
            raise ValueError("read_starts and read_ends must hold one byte offset per read, 0 <= read_starts[s] <= read_ends[s] <= len(seq)" if every else
                             "read_ends must hold one byte offset per read, read_starts[s] <= read_ends[s] <= len(seq)")

    def on(self, xp):
        """(starts, ends) as int64 columns of the namespace xp, unchecked: a column that is a CUDA tensor already stays on its device,
        anything else is uploaded once; default ends are made where read_starts lives"""
        cuda = lambda x: not xp.host and _is_tensor(x) and x.is_cuda      # noqa: E731
        starts = self.read_starts.long().ravel() if cuda(self.read_starts) else xp.place(self.host[0])
        if cuda(self.read_ends):
            return starts, self.read_ends.long().ravel()
        if self.read_ends is None and cuda(self.read_starts):
            return starts, xp.concat([starts[1:], xp.place(np.array([self.n_text], dtype=np.int64))])
        return starts, xp.place(self.host[1])


def read_segments(xp, q, layout):
    """the segment CSR of the reads over the anchors' query positions q, which ascend (no read_starts: one read, no CSR): read s owns the
    anchors with read_starts[s] <= qpos < read_starts[s + 1]"""
    if layout.read_starts is None:
        return None
    layout.ascending()
    return xp.narrow(xp.concat([xp.searchsorted(xp.signed(q), xp.place(layout.host[0])), xp.place(np.array([len(q)], dtype=np.int64))]), np.uint64)


def chain_rows(xp, q, r, v, c, k, seg=None, groups=None):
    """the per-chain columns of a ChainTable (seg, rev, q_start, q_end, r_start, r_end, count, score) from the first and last anchor of
    every chain of c (a Chains).  seg: the CSR chain_anchors chained under -- of reads, or with groups (an AnchorGroups) of (read, target)
    groups, whose read groups.seg names"""
    first, last = xp.signed(c.first), xp.signed(c.last)
    qf, ql, rf, rl = q[first], q[last], r[first], r[last]
    sg = xp.full(len(first), 0, np.uint32) if seg is None else xp.narrow(xp.searchsorted(seg, first, right=True) - 1, np.uint32)
    if groups is not None:
        sg = groups.seg[xp.signed(sg)]
    return sg, v[first], qf, ql + k, xp.minimum(rf, rl), xp.maximum(rf, rl) + k, c.count, c.cscore


def chain_read_intervals(xp, layout, seg):
    """(q_lo, q_hi) per chain: the byte interval of the read table.seg names, as chain_ends and chain_records take it"""
    sg = xp.signed(seg)
    return tuple(xp.narrow(xp.place(h)[sg], np.uint32) for h in layout.host)


def seg_offsets(xp, seg, n_reads, checked):
    """read g owns the rows with seg == g, and seg does not descend: offsets[g] = the first row with seg >= g, n_reads + 1 entries.
    checked: ValueError where a row names a read at or beyond n_reads (reads a value: on a device column that is a wait)"""
    offs = xp.narrow(xp.searchsorted(xp.signed(seg), xp.arange(n_reads + 1)), np.uint64)
    if checked and int(offs[-1]) != len(seg):
        raise ValueError("n_reads = %d does not cover the reads of the table (seg reaches %d)" % (n_reads, int(xp.signed(seg).max())))
    return offs


def printable(xp, mapping, targets=None, kept_only=True):
    """the printable-row rule of write_paf, the SAM writers and pairing: kept by select (with kept_only), valid, and with targets inside
    one of them -> (printable, considered: the rows kept_only lets through, target per row or None)"""
    sel, rec = mapping.select, mapping.records
    flag, valid = xp.col(sel.flag, np.uint8), xp.col(rec.valid, np.uint8)
    considered = (flag & FLAG_KEPT) != 0 if kept_only else xp.full(len(valid), 1, np.uint8) != 0
    good, tgt = considered & (valid != 0), None
    if targets is not None:      # a row's target is the one its first reference base lies in; its end must lie there too
        inside, tgt = inside_target(xp, targets, xp.col(rec.rs, np.uint32), xp.col(rec.re, np.uint32))
        good = good & inside
    return good, considered, tgt


def pair_candidates(xp, mapping, n_reads, targets=None):
    """the arguments pair_mapping derives for pair_chains -> (read_offsets, use, tid or None); a host Mapping is checked against n_reads"""
    offs = seg_offsets(xp, mapping.table.seg, n_reads, checked=xp.host)
    use, _, tgt = printable(xp, mapping, targets)
    tid = None if tgt is None else xp.narrow(tgt, np.uint32)      # (-1 holds the bits of KH_TARGET_NONE)
    return offs, xp.narrow(use, np.uint8), tid


def rescue_windows(xp, mapping, pairs, layout, min_ins, max_ins, max_edits, targets=None, ref_len=None, ref_base=0):
    """the body of rescue_requests(), which holds the definition, over checked integer parameters"""
    rec = mapping.records
    row, trev = xp.col(pairs.row, np.int32), xp.col(mapping.table.rev, np.uint8)
    n_reads = len(row)
    if n_reads % 2:
        raise ValueError("reads come in pairs (mate 1, mate 2, ...): an even number of reads is needed, got %d" % n_reads)
    starts, ends = layout.on(xp)
    if len(starts) != n_reads or len(ends) != n_reads:
        raise ValueError("read_starts and read_ends must hold one entry per read of pairs (%d), got %d and %d" % (n_reads, len(starts), len(ends)))
    const = lambda v: xp.full(n_reads, v)      # noqa: E731
    own, n_rows = xp.signed(row), len(rec.rs)
    prow = own[xp.arange(n_reads) ^ 1]
    need = (own == -1) & (prow >= 0) & (prow < n_rows)
    if n_rows == 0 or n_reads == 0:
        return RescueRequests(*(xp.narrow(xp.full(0, 0), dt) for dt in (np.uint32, np.uint32, np.uint32, np.uint32, np.uint8, np.uint32)))
    at = xp.where(need, prow, const(0))
    prs, pre = (xp.widen(xp.col(x, np.uint32))[at] for x in (rec.rs, rec.re))
    fwd = (xp.signed(trev)[at] & 1) == 0
    if targets is not None:
        tgt, _ = targets.locate_on(xp, prs)
        need = need & (tgt >= 0)
        tc = xp.where(tgt >= 0, tgt, const(0))
        tlo, thi = targets.bound(xp, 0)[tc], targets.bound(xp, 1)[tc]
    else:
        tlo, thi = const(ref_base), const(int(ref_base) + int(ref_len))
    m = ends - starts
    w_lo = xp.where(fwd, xp.maximum(prs, prs + (min_ins - max_edits) - m), pre - max_ins)
    w_hi = xp.where(fwd, prs + max_ins, xp.minimum(pre, pre - (min_ins - max_edits) + m))
    w_lo = xp.minimum(xp.maximum(w_lo, tlo), thi)
    w_hi = xp.maximum(xp.minimum(w_hi, thi), w_lo)
    w_hi = xp.where(fwd, xp.minimum(w_hi, w_lo + RESCUE_MAX_WINDOW), w_hi)
    w_lo = xp.where(fwd, w_lo, xp.maximum(w_lo, w_hi - RESCUE_MAX_WINDOW))
    sel = xp.nonzero(need)      # (on the device the one wait: the number of requests)
    return RescueRequests(*(xp.narrow(x[sel], np.uint32) for x in (starts, ends, w_lo, w_hi)), xp.narrow(fwd[sel], np.uint8), xp.narrow(sel, np.uint32))


# ---- the pipeline: plain functions of a stranded index ix (the methods of KmerPositionIndex, which hold the documentation, delegate here) ----
def _check_targets_text(targets, ref_text, ref_base, max_edits):
    """the refusals of the calls that read the reference text of a multi-target index: the text must be the one the Targets lay out, from
    coordinate 0, and no alignment may afford a spacer"""
    if not isinstance(targets, Targets):
        raise ValueError("targets must be a kmerhash_amd.Targets where the reference text is read, got %r" % (type(targets).__name__,))
    if targets.spacer <= int(max_edits):
        raise ValueError("the spacer between targets (%d) must exceed max_edits (%r): an alignment could cross it" % (targets.spacer, max_edits))
    if int(ref_base) != 0:
        raise ValueError("ref_base must be 0 with targets (their coordinates are those of the whole text), got %r" % (ref_base,))
    n = _Buf.text(ref_text).n
    if n != int(targets.ends[-1]):
        raise ValueError("ref_text must be the text the targets lay out (%d bytes), got %d" % (int(targets.ends[-1]), n))


def _chains(ix, seq, layout, params, targets=None):
    """-> (ChainTable, the Chains chain_anchors returned: pred per anchor, first and last anchor per chain)"""
    q, r, v = ix.anchors(seq)
    xp = namespace_of(q)
    seg = read_segments(xp, q, layout)
    groups = None
    if targets is not None:      # chain per (read, target): the group CSR takes the place of the read CSR
        groups = group_anchors(q, r, v, targets, ix.k, seg, ix.device)
        q, r, v, seg = groups.qpos, groups.rpos, groups.rev, groups.offsets
    c = chain_anchors(q, r, v, ix.k, seg, device=ix.device, **params)
    return ChainTable(*chain_rows(xp, q, r, v, c, ix.k, seg, groups), (q, r, v), c.chain), c


def chains(ix, seq, read_starts=None, targets=None, **params):
    return _chains(ix, seq, ReadLayout(read_starts, None, None), params, targets)[0]


def _verify(ix, seq, ref_text, layout, ref_base, max_edits, clip_cost, params, targets, stages):
    """the chains of seq verified against the texts, `stages` deep: 1 chain_edits, 2 chain_cigars too, 3 chain_ends too
    -> (ChainTable, ChainEdits, ChainCigars, ChainEnds, the Chains of chain_anchors, q_lo, q_hi per chain), None for what was not asked"""
    if targets is not None:
        _check_targets_text(targets, ref_text, ref_base, max_edits)
    seq = _Buf.text(seq).obj          # (bytes as an array: the text goes to several calls)
    table, c = _chains(ix, seq, layout, params, targets)
    q, r, v = table.anchors
    n_chains = len(table.count)
    lo = hi = cigars = ends = None
    if stages == 3:
        layout.bounded(every=False)
        lo, hi = chain_read_intervals(namespace_of(q), layout, table.seg)
    edits = chain_edits(seq, ref_text, q, r, v, c.pred, table.chain, n_chains, ix.k, ref_base, max_edits, ix.device)
    if stages >= 2:
        cigars = chain_cigars(seq, ref_text, q, r, v, c.pred, table.chain, n_chains, ix.k, edits.link, ref_base, ix.device)
    if stages == 3:
        ends = chain_ends(seq, ref_text, q, r, v, c.first, c.last, lo, hi, ix.k, ref_base, max_edits, clip_cost, ix.device)
    return table, edits, cigars, ends, c, lo, hi


def index_chain_edits(ix, seq, ref_text, read_starts=None, ref_base=0, max_edits=31, targets=None, **params):
    return _verify(ix, seq, ref_text, ReadLayout.of(seq, read_starts), ref_base, max_edits, 4, params, targets, 1)[:2]


def index_chain_cigars(ix, seq, ref_text, read_starts=None, ref_base=0, max_edits=31, targets=None, **params):
    return _verify(ix, seq, ref_text, ReadLayout.of(seq, read_starts), ref_base, max_edits, 4, params, targets, 2)[:3]


def index_chain_ends(ix, seq, ref_text, read_starts=None, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, targets=None, **params):
    return _verify(ix, seq, ref_text, ReadLayout.of(seq, read_starts, read_ends), ref_base, max_edits, clip_cost, params, targets, 3)[:4]


def chain_select(ix, seq, read_starts=None, mask_pct=50, pri_pct=80, best_n=5, **params):
    targets = params.pop("targets", None)
    layout = ReadLayout(read_starts, None, None)
    table = _chains(ix, seq, layout, params, targets)[0]
    return table, select_table(table, layout.n_reads, mask_pct=mask_pct, pri_pct=pri_pct, best_n=best_n, device=ix.device)


def map_reads(ix, seq, ref_text, read_starts=None, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, mask_pct=50, pri_pct=80, best_n=5, ref_order=True,
              targets=None, **params):
    layout = ReadLayout.of(seq, read_starts, read_ends)
    table, edits, cigars, ends, c, lo, hi = _verify(ix, seq, ref_text, layout, ref_base, max_edits, clip_cost, params, targets, 3)
    select = select_table(table, layout.n_reads, mask_pct=mask_pct, pri_pct=pri_pct, best_n=best_n, device=ix.device)
    q, r, v = table.anchors
    records = chain_records(q, r, v, table.chain, cigars, c.first, c.last, lo, hi, ends, ix.k, ref_order, ix.device)
    return Mapping(table, edits, cigars, ends, select, records)


def map_pairs(ix, seq, ref_text, read_starts, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, mask_pct=50, pri_pct=80, best_n=5,
              min_ins=0, max_ins=1000, unpaired_pen=17, targets=None, **params):
    layout = ReadLayout.of(seq, read_starts, read_ends)
    n_reads = layout.n_reads
    if n_reads % 2:
        raise ValueError("reads come in pairs (mate 1, mate 2, ...): an even number of reads is needed, got %d" % n_reads)
    mp = map_reads(ix, seq, ref_text, layout, None, ref_base, max_edits, clip_cost, mask_pct, pri_pct, best_n, True, targets, **params)
    return mp, pair_mapping(mp, n_reads, targets, min_ins=min_ins, max_ins=max_ins, unpaired_pen=unpaired_pen, device=ix.device)


def map_pairs_rescued(ix, seq, ref_text, read_starts, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, mask_pct=50, pri_pct=80, best_n=5,
                      min_ins=0, max_ins=1000, unpaired_pen=17, targets=None, **params):
    layout = ReadLayout.of(seq, read_starts, read_ends)
    mp, pairs = map_pairs(ix, seq, ref_text, layout, None, ref_base, max_edits, clip_cost, mask_pct, pri_pct, best_n, min_ins, max_ins, unpaired_pen, targets, **params)
    sb, rb = _Buf.text(seq), _Buf.text(ref_text)
    rq = rescue_windows(namespace_of(pairs.row), mp, pairs, layout, int(min_ins), int(max_ins), int(max_edits), targets, rb.n, ref_base)
    res = rescue_mates(sb.obj, rb.obj, rq.q_lo, rq.q_hi, rq.w_lo, rq.w_hi, rq.rev, ref_base, max_edits, ix.device)
    return mp, pairs, res._replace(read=rq.read)


def map_fastq(ix, text, ref_text, strict=True, strip_mate=None, **kw):
    reads = read_fastq(text, None, strict, strip_mate, ix.device)
    return map_reads(ix, reads.seq, ref_text, reads.read_starts, reads.read_ends, **kw), reads


def map_fastq_pairs(ix, text, ref_text, text2=None, rescue=False, strict=True, strip_mate=None, **kw):
    reads = read_fastq(text, text2, strict, strip_mate, ix.device)
    return (map_pairs_rescued if rescue else map_pairs)(ix, reads.seq, ref_text, reads.read_starts, reads.read_ends, **kw) + (reads,)
