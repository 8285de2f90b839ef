"""SAM output of a Mapping (index.map): the difference strings MD:Z: and cs:Z: and the reads in reference orientation come from the
device (kh_record_diffs, kh_oriented_rows in include/kmerhash_amd.h, which holds the definitions); the header, the flags and the
lines are host formatting beside kmers.paf_lines."""
import collections

import numpy as np

from . import _capi as K
from ._call import _Buf, _is_tensor, alloc, check_same, two_pass
from ._xp import NUMPY, namespace_of
from .mapper import FLAG_PRIMARY, ChainRecords, Mapping, ReadLayout, _host, chain_read_intervals, cigar_text, printable as printable_rows
from .targets import inside_target

RecordDiffs = collections.namedtuple("RecordDiffs", "ok offsets text")
DIFF_KINDS = {"cs": 0, "md": 1}      # KH_DIFF_CS, KH_DIFF_MD


def record_diffs(qtext, rtext, records, rev, q_lo, q_hi, kind="cs", ref_base=0, device=0):
    """which bases the X, I and D runs of every record were (kh_record_diffs): per row of `records` (a ChainRecords made with
    ref_order=True) the short cs string (kind="cs": ':' matches, '*' reference base and read base, '+' inserted, '-' deleted bases, lower
    case) or the MD string of SAM (kind="md").  qtext and rtext are the texts the records were made from, rtext covering the reference
    coordinates [ref_base, ref_base + len(rtext)); rev (bit 0: the strand, table.rev), q_lo and q_hi (the byte interval of each row's
    read in qtext) hold one entry per row.
    -> RecordDiffs(ok, offsets, text): ok[c] = 1 where the row walks the two texts from end to end (an invalid row, or one that does not
    fit its read or the reference text, has ok 0 and no text); row c is text[offsets[c]:offsets[c + 1]].  numpy in, numpy out (uint8,
    uint64, uint8); CUDA tensors in, tensors out on the current stream (int64 offsets, uint8 text); count, then emit, one wait per pass."""
    if kind not in DIFF_KINDS:
        raise ValueError("kind must be 'cs' or 'md', got %r" % (kind,))
    qb, rb = _Buf.text(qtext), _Buf.text(rtext)
    ob, pb, vb, sb = _Buf(records.offsets, np.uint64), _Buf(records.ops, np.uint32), _Buf(records.valid, np.uint8), _Buf(records.rs, np.uint32)
    eb, lb, hb = _Buf(rev, np.uint8), _Buf(q_lo, np.uint32), _Buf(q_hi, np.uint32)
    check_same("the texts, the records, rev, q_lo and q_hi must live in the same memory", qb, rb, ob, pb, vb, sb, eb, lb, hb, length=False)
    rows = vb.n
    check_same("records.valid, records.rs, rev, q_lo and q_hi must have one entry per row, got %d, %d, %d, %d and %d" % (rows, sb.n, eb.n, lb.n, hb.n), vb, sb, eb, lb, hb)
    if ob.n != rows + 1:
        raise ValueError("records.offsets must hold one entry per row and one more, got %d for %d rows" % (ob.n, rows))
    if rows > 2 ** 31 or pb.n > 2 ** 31 or qb.n > 2 ** 32 or rb.n > 2 ** 32 or not 0 <= int(ref_base) < 2 ** 32:
        raise ValueError("at most 2^31 rows and runs and texts of 2^32 bytes per call, ref_base a u32")
    ok, kptr = alloc(vb, rows, np.uint8, empty=True)
    offs, optr = alloc(vb, rows + 1, np.uint64, zero=True)
    if rows == 0:      # nothing to queue: the zeroed offset is the answer
        return RecordDiffs(ok, offs, alloc(vb, 0, np.uint8)[0])
    args = (qb.ptr_or_null, qb.n, rb.ptr_or_null, rb.n, int(ref_base), ob.ptr, pb.ptr_or_null, pb.n, vb.ptr, eb.ptr, lb.ptr, hb.ptr, sb.ptr, rows, DIFF_KINDS[kind], vb.where,
            kptr, optr)
    return RecordDiffs(ok, offs, two_pass("kh_record_diffs", args, vb, np.uint8, device))


def oriented_rows(text, lo, hi, rev, complement=True, device=0):
    """byte ranges of a text as rows in reference orientation (kh_oriented_rows): row c is text[lo[c]:hi[c]] (clamped to the text, empty
    where hi <= lo) as it stands where bit 0 of rev[c] is clear and back to front where it is set -- with complement every base of a
    reversed row complemented (A<->T, C<->G, case kept, any other byte itself): SEQ; without, reversed only: QUAL.
    -> (offsets, text): row c is text[offsets[c]:offsets[c + 1]].  numpy in, numpy out (uint64, uint8); CUDA tensors in, tensors out on
    the current stream (int64, uint8); count, then emit, one wait per pass."""
    tb, lb, hb, eb = _Buf.text(text), _Buf(lo, np.uint32), _Buf(hi, np.uint32), _Buf(rev, np.uint8)
    check_same("text, lo, hi and rev must live in the same memory", tb, lb, hb, eb, length=False)
    check_same("lo, hi and rev must have one entry per row, got %d, %d and %d" % (lb.n, hb.n, eb.n), lb, hb, eb)
    rows = lb.n
    if rows > 2 ** 31 or tb.n > 2 ** 32:
        raise ValueError("at most 2^31 rows and a text of 2^32 bytes per call, got %d and %d" % (rows, tb.n))
    offs, optr = alloc(lb, rows + 1, np.uint64, zero=True)
    if rows == 0:
        return offs, alloc(lb, 0, np.uint8)[0]
    args = (tb.ptr_or_null, tb.n, lb.ptr, hb.ptr, eb.ptr, rows, 1 if complement else 0, lb.where, optr)
    return offs, two_pass("kh_oriented_rows", args, lb, np.uint8, device)


def sam_header(targets=None, ref_name=None, ref_len=None):
    """the header of a SAM file as one string: @HD VN:1.6 SO:unsorted, one @SQ per target (targets: a kmerhash_amd.Targets; or the one
    reference ref_name / ref_len), @PG with the library's version"""
    if targets is not None:
        if ref_name is not None or ref_len is not None:
            raise ValueError("with targets the names and lengths are theirs: ref_name and ref_len must be None")
        sq = [(n, int(l)) for n, l in zip(targets.names, targets.lengths)]
    elif ref_name is None or ref_len is None:
        raise ValueError("ref_name and ref_len are needed without targets")
    else:
        sq = [(str(ref_name), int(ref_len))]
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % s for s in sq]
    lines.append("@PG\tID:kmerhash_amd\tPN:kmerhash_amd\tVN:%s" % K.lib().kh_version().decode())
    return "".join(l + "\n" for l in lines)


def _mapped_reads(mapping, printable):
    """per read: is select.best[s] a printable row?"""
    best = _host(mapping.select.best, np.int32).astype(np.int64)
    inside = (best >= 0) & (best < len(printable))
    return inside & printable[np.where(inside, best, 0)] if len(printable) else np.zeros(len(best), dtype=bool)


ROLE_REP, ROLE_SUPP, ROLE_SEC = 1, 2, 3      # what a printable row of a paired read is printed as: the representative, 0x800, 0x100


def _pair_roles(mapping, pairs, printable):
    """paired output: -> (rep, role): rep[s] = the row that represents read s -- pairs.row[s] where that is a printable row of the read,
    else -1 (unmapped) --; role[c] of every printable row of a mapped read: ROLE_REP for the representative, ROLE_SEC for a row that is
    a secondary in select or the select.parent of the representative, ROLE_SUPP for any other; 0 for the rows that are not printed"""
    seg, flag = _host(mapping.table.seg, np.uint32).astype(np.int64), _host(mapping.select.flag, np.uint8)
    parent = _host(mapping.select.parent, np.int32).astype(np.int64)
    row = _host(pairs.row, np.int32).astype(np.int64)
    n_rows, n_reads = len(flag), len(row)
    if n_rows == 0:
        return np.full(n_reads, -1, dtype=np.int64), np.zeros(0, dtype=np.uint8)
    inside = (row >= 0) & (row < n_rows)
    at = np.where(inside, row, 0)
    rep = np.where(inside & printable[at] & (seg[at] == np.arange(n_reads)), row, -1)
    own = np.where(seg < n_reads, rep[np.minimum(seg, max(n_reads - 1, 0))], -1) if n_reads else np.full(n_rows, -1, dtype=np.int64)
    shown = printable & (own >= 0)
    c = np.arange(n_rows)
    sec = ((flag & FLAG_PRIMARY) == 0) | (c == parent[np.maximum(own, 0)])
    role = np.where(c == own, ROLE_REP, np.where(sec, ROLE_SEC, ROLE_SUPP)).astype(np.uint8)
    return rep, np.where(shown, role, 0).astype(np.uint8)


def _rows_of(pair):
    offs, text = pair
    return _host(offs, np.int64), _host(text, np.uint8).tobytes().decode("latin-1")


def sam_lines(mapping, text_offsets, text, seq_rows, read_names, qual_rows=None, md=None, cs=None, ref_name=None, ref_len=None, ref_start=0, targets=None,
              kept_only=True, unmapped=True, header=True, pairs=None):
    """the formatting half of write_sam() (host only).  text_offsets, text: the CIGAR text CSR of the record rows (cigar_text); md, cs:
    RecordDiffs of the two kinds or None; seq_rows (and qual_rows, or None): an (offsets, text) CSR of n_rows + n_reads rows -- row c
    the oriented read of table row c (needed for the primary rows that are printed), row n_rows + s read s as given (needed for the
    unmapped reads).  pairs: the PairSelect of the reads (see write_sam_pairs), whose representatives and 0x800 rows then need their seq_rows.
    -> (lines, skipped, unmapped_reads): the header lines first when `header`."""
    return _sam_lines(mapping, text_offsets, text, seq_rows, read_names, qual_rows, md, cs, ref_name, ref_len, ref_start, targets, kept_only, unmapped, header, pairs, None)


def _tlen(s, own, mate):
    """the template-length rule of kh_pair_chains over the intervals (rs, re) of read s and of its mate"""
    t = min(max(own[1], mate[1]) - min(own[0], mate[0]), 2 ** 31 - 1)
    return t if own[0] < mate[0] or (own[0] == mate[0] and s % 2 == 0) else -t


def _sam_lines(mapping, text_offsets, text, seq_rows, read_names, qual_rows, md, cs, ref_name, ref_len, ref_start, targets, kept_only, unmapped, header, pairs, rescued):
    """the body of sam_lines(); rescued (paired output only): {read: the alignment mate rescue gave it} as _write_sam builds it, or None"""
    if targets is not None and int(ref_start) != 0:
        raise ValueError("with targets the starts are theirs: ref_start must be 0")
    head = sam_header(targets, ref_name, ref_len).splitlines()      # (checks ref_name / ref_len against targets)
    t, sel, rec = mapping.table, mapping.select, mapping.records
    seg, rev, count, score = _host(t.seg, np.uint32), _host(t.rev, np.uint8), _host(t.count, np.uint32), _host(t.score, np.int32)
    flag, mapq, sub, best = _host(sel.flag, np.uint8), _host(sel.mapq, np.uint8), _host(sel.sub, np.int32), _host(sel.best, np.int32)
    rs, re_, nm = _host(rec.rs, np.uint32), _host(rec.re, np.uint32), _host(rec.nm, np.uint32)
    n_rows, n_reads = len(flag), len(best)
    rescued = rescued or {}
    printable, considered, tgt = printable_rows(NUMPY, mapping, targets, kept_only)
    mapped = _mapped_reads(mapping, printable) if pairs is None else None      # (paired: the representatives say who is mapped)
    toff, raw = _rows_of((text_offsets, text))
    soff, sraw = _rows_of(seq_rows)
    qoff, qraw = _rows_of(qual_rows) if qual_rows is not None else (None, None)
    diffs = [(tag, _host(d.ok, np.uint8), *_rows_of((d.offsets, d.text))) for tag, d in (("MD", md), ("cs", cs)) if d is not None]
    if len(soff) != n_rows + n_reads + 1 or (qoff is not None and len(qoff) != len(soff)):
        raise ValueError("seq_rows and qual_rows must hold one row per table row and one per read")
    rows_of = [[] for _ in range(n_reads)]
    for c in np.flatnonzero(considered):
        if int(seg[c]) < n_reads:
            rows_of[int(seg[c])].append(int(c))
    lines, skipped, n_unmapped = (list(head) if header else []), 0, 0
    if pairs is not None:
        pmapq, ptlen, pflag = _host(pairs.mapq, np.uint8), _host(pairs.tlen, np.int32), _host(pairs.flag, np.uint8)
        if n_reads % 2 or any(len(x) != n_reads for x in (_host(pairs.row, np.int32), pmapq, ptlen)) or len(pflag) != n_reads // 2:
            raise ValueError("pairs must hold one entry per read of the Mapping (row, mapq, tlen) and one per pair (flag), and the reads must come in pairs")
        rep, role = _pair_roles(mapping, pairs, printable)

        def place(c):      # -> (target number, RNAME, POS) of row c
            if targets is None:
                return 0, str(ref_name), int(rs[c]) - int(ref_start) + 1
            return int(tgt[c]), targets.names[int(tgt[c])], int(rs[c]) - int(targets.starts[int(tgt[c])]) + 1

        for s in range(n_reads):
            name, r, mr = str(read_names[s]), int(rep[s]), int(rep[s ^ 1])
            me, mate = rescued.get(s), rescued.get(s ^ 1)      # the alignment mate rescue gave this read / its mate (then r < 0 <= mr / mr < 0 <= r)
            if me is not None:      # printed as mapped: a concordant pair by construction
                x = n_rows + s
                pt, pname, ppos = place(mr)
                fl = 0x1 | (0x80 if s & 1 else 0x40) | 0x2 | (0x10 if me["rev"] else 0) | (0x20 if rev[mr] & 1 else 0)
                f = [name, fl, me["tname"], me["pos"], me["mapq"], me["cigar"], "=" if pt == me["tn"] else pname, ppos,
                     _tlen(s, (me["rs"], me["re"]), (int(rs[mr]), int(re_[mr]))) if pt == me["tn"] else 0, sraw[soff[x]:soff[x + 1]] or "*",
                     (qraw[qoff[x]:qoff[x + 1]] if qraw is not None else "") or "*", "NM:i:%d" % me["nm"], "tp:A:R"] + me["tags"]
                skipped += len(rows_of[s])
                lines.append("\t".join(str(v) for v in f))
                continue
            fl0 = 0x1 | (0x80 if s & 1 else 0x40)
            if mate is not None:
                fl0 |= 0x20 if mate["rev"] else 0
            else:
                fl0 |= 0x8 if mr < 0 else (0x20 if rev[mr] & 1 else 0)
            at = mr if mr >= 0 else r      # (an unmapped mate is placed at this read's representative: the mate columns point there)
            mt, mname, mpos = place(at) if at >= 0 else (-1, "*", 0)
            if mate is not None:
                mt, mname, mpos = mate["tn"], mate["tname"], mate["pos"]
            both = r >= 0 and mr >= 0      # (0x2 and TLEN need both representatives: a PairSelect made under other targets or kept_only may name a row that is not printed)
            if r < 0:
                n_unmapped += 1
                skipped += len(rows_of[s])
                if unmapped:      # at the mate's place, as the SAM specification recommends
                    x = n_rows + s
                    lines.append("\t".join([name, str(fl0 | 0x4), mname, str(mpos), "0", "*", "=" if mr >= 0 else "*", str(mpos), "0", sraw[soff[x]:soff[x + 1]] or "*",
                                            (qraw[qoff[x]:qoff[x + 1]] if qraw is not None else "") or "*"]))
                continue
            for c in rows_of[s]:
                if not printable[c]:
                    skipped += 1
                    continue
                is_rep, pri = c == r, role[c] != ROLE_SEC
                proper = is_rep and (mate is not None or (both and pflag[s >> 1] & 1))
                fl = fl0 | (0x10 if rev[c] & 1 else 0) | {ROLE_REP: 0, ROLE_SUPP: 0x800, ROLE_SEC: 0x100}[int(role[c])] | (0x2 if proper else 0)
                tn, tname, pos = place(c)
                tlen = int(ptlen[s]) if is_rep and both else 0
                if is_rep and mate is not None and mt == tn:
                    tlen = _tlen(s, (int(rs[c]), int(re_[c])), (mate["rs"], mate["re"]))
                f = [name, fl, tname, pos, int(pmapq[s]) if is_rep else int(mapq[c]), raw[toff[c]:toff[c + 1]], "=" if mt == tn else mname, mpos,
                     tlen, (sraw[soff[c]:soff[c + 1]] if pri else "") or "*", (qraw[qoff[c]:qoff[c + 1]] if pri and qraw is not None else "") or "*",
                     "NM:i:%d" % int(nm[c]), "tp:A:%s" % ("P" if pri else "S"), "cm:i:%d" % int(count[c]), "s1:i:%d" % int(score[c])]
                if pri:
                    f.append("s2:i:%d" % int(sub[c]))
                for tag, ok, doff, draw in diffs:
                    if not ok[c]:
                        raise ValueError("row %d does not walk the two texts: make the Mapping with ref_order=True and pass the texts it was made from" % c)
                    f.append("%s:Z:%s" % (tag, draw[doff[c]:doff[c + 1]]))
                lines.append("\t".join(str(x) for x in f))
        return lines, skipped, n_unmapped
    for s in range(n_reads):
        name = str(read_names[s])
        if not mapped[s]:
            n_unmapped += 1
            skipped += len(rows_of[s])
            if unmapped:
                r = n_rows + s
                lines.append("\t".join([name, "4", "*", "0", "0", "*", "*", "0", "0", sraw[soff[r]:soff[r + 1]] or "*",
                                        (qraw[qoff[r]:qoff[r + 1]] if qraw is not None else "") or "*"]))
            continue
        for c in rows_of[s]:
            if not printable[c]:
                skipped += 1
                continue
            pri = bool(flag[c] & FLAG_PRIMARY)
            fl = (0x10 if rev[c] & 1 else 0) | (0 if pri else 0x100) | (0x800 if pri and c != int(best[s]) else 0)
            if targets is None:
                tname, t0 = str(ref_name), int(ref_start)
            else:
                tname, t0 = targets.names[int(tgt[c])], int(targets.starts[int(tgt[c])])
            f = [name, fl, tname, int(rs[c]) - t0 + 1, int(mapq[c]), raw[toff[c]:toff[c + 1]], "*", 0, 0,
                 (sraw[soff[c]:soff[c + 1]] if pri else "") or "*", (qraw[qoff[c]:qoff[c + 1]] if pri and qraw is not None else "") or "*",
                 "NM:i:%d" % int(nm[c]), "tp:A:%s" % ("P" if pri else "S"), "cm:i:%d" % int(count[c]), "s1:i:%d" % int(score[c])]
            if pri:
                f.append("s2:i:%d" % int(sub[c]))
            for tag, ok, doff, draw in diffs:
                if not ok[c]:
                    raise ValueError("row %d does not walk the two texts: make the Mapping with ref_order=True and pass the texts it was made from" % c)
                f.append("%s:Z:%s" % (tag, draw[doff[c]:doff[c + 1]]))
            lines.append("\t".join(str(x) for x in f))
    return lines, skipped, n_unmapped


def _host_columns(mapping, parent=False):
    """the per-row columns of a Mapping on the host, copied once (the CSRs stay where they are); parent: select.parent too"""
    t, sel, rec = mapping.table, mapping.select, mapping.records
    h = lambda x, dt: _host(x, dt)      # noqa: E731
    table = t._replace(seg=h(t.seg, np.uint32), rev=h(t.rev, np.uint8), count=h(t.count, np.uint32), score=h(t.score, np.int32))
    select = sel._replace(flag=h(sel.flag, np.uint8), mapq=h(sel.mapq, np.uint8), sub=h(sel.sub, np.int32), best=h(sel.best, np.int32))
    if parent:
        select = select._replace(parent=h(sel.parent, np.int32))
    records = rec._replace(valid=h(rec.valid, np.uint8), rs=h(rec.rs, np.uint32), re=h(rec.re, np.uint32), nm=h(rec.nm, np.uint32))
    return Mapping(table, mapping.edits, mapping.cigars, mapping.ends, select, records)


def write_sam(fh, mapping, seq, ref_text, read_names, read_starts, read_ends=None, qual=None, ref_name=None, ref_len=None, ref_start=0, ref_base=0, targets=None,
              kept_only=True, unmapped=True, header=True, md=True, cs=False, device=0):
    """the rows of a Mapping (index.map) as a SAM file into the text file `fh`.  On the device: one cigar_text() call over the records,
    one record_diffs() call per difference string asked for (md: MD:Z:, cs: the short cs:Z:), one oriented_rows() call for SEQ and one
    for QUAL when `qual` is given; then one copy of the columns to the host and one line per row (sam_lines).
    seq, ref_text: the texts the Mapping was made from (ref_text covers [ref_base, ref_base + len)), living where the Mapping lives;
    read_starts / read_ends: the byte interval of every read in seq, as index.map took them; qual: a text like seq in which qual[i] is
    the quality of seq[i]; read_names[s]: the name of read s.  One target (ref_name, ref_len) whose base 0 is reference coordinate
    ref_start, or targets: the kmerhash_amd.Targets the Mapping was made with (then ref_name / ref_len / ref_start stay None / None / 0).
    A row is printable under the rules of write_paf: kept (with kept_only), valid, inside one target.  Read s is represented by row
    select.best[s]: where that row is missing or not printable the read is written as unmapped (flag 4, the read as given) -- or
    dropped with unmapped=False -- and its other printable rows count as skipped; otherwise every printable row of the read gives a
    line: QNAME, FLAG (0x10 reverse strand, 0x100 secondary, 0x800 a primary other than best[s]), RNAME, POS = rs - start + 1, MAPQ,
    CIGAR (S I D = X), * 0 0, SEQ and QUAL in reference orientation ('*' for secondaries, QUAL '*' without qual), then NM:i, tp:A:P|S,
    cm:i, s1:i, s2:i (primaries), MD:Z, cs:Z.  Lines are grouped by read, reads ascending, a read's rows in table order.
    Make the Mapping with ref_order=True: SAM wants the CIGAR of a reverse-strand row in reference order, and so do the difference
    strings -- a row that does not walk the texts raises ValueError.
    write_sam_pairs() writes the same file with the mate columns of paired reads.
    -> (alignment lines written, rows skipped, unmapped reads)"""
    return _write_sam(fh, mapping, seq, ref_text, read_names, read_starts, read_ends, qual, ref_name, ref_len, ref_start, ref_base, targets, kept_only, unmapped, header, md, cs,
                      device, None)


def write_sam_pairs(fh, mapping, pairs, seq, ref_text, read_names, read_starts, read_ends=None, qual=None, ref_name=None, ref_len=None, ref_start=0, ref_base=0,
                    targets=None, kept_only=True, unmapped=True, header=True, md=True, cs=False, device=0):
    """write_sam() for paired reads: the same device calls, texts and arguments, and the mate columns filled from
    pairs: the PairSelect of index.map_pairs / kmers.pair_mapping over this Mapping (reads interleaved mate 1, mate 2, ...).
    Read s is represented by row pairs.row[s] (unmapped where that is -1 or not
    printable) and that line carries pairs.mapq[s] and TLEN = pairs.tlen[s]; another printable row of the read is printed 0x100 if
    select made it a secondary or if it is the select.parent of the representative, else 0x800; SEQ, QUAL and tp:A:P go to the
    representative and the 0x800 rows.  Every line has 0x1 and 0x40 / 0x80 by mate number, 0x20 where the mate's representative is on
    the reverse strand, 0x8 where the mate is unmapped, and RNEXT / PNEXT = the mate's representative's target ('=' for the line's own)
    and POS; 0x2 is set on the representatives of a proper pair.  An unmapped read whose mate is mapped stands at the mate's RNAME /
    POS, with RNEXT '=' and the same PNEXT, and the mate's own RNEXT / PNEXT point there too; two unmapped mates keep * 0 ... * 0 0.
    Names are printed as given.  write_sam() itself is unchanged: it knows nothing of pairs and writes what it wrote.
    -> (alignment lines written, rows skipped, unmapped reads)"""
    if pairs is None:
        raise ValueError("write_sam_pairs() needs a PairSelect; write_sam() writes unpaired reads")
    return _write_sam(fh, mapping, seq, ref_text, read_names, read_starts, read_ends, qual, ref_name, ref_len, ref_start, ref_base, targets, kept_only, unmapped, header, md, cs,
                      device, pairs)


def write_sam_rescued(fh, mapping, pairs, rescue, seq, ref_text, read_names, read_starts, read_ends=None, qual=None, ref_name=None, ref_len=None, ref_start=0, ref_base=0,
                      targets=None, kept_only=True, unmapped=True, header=True, md=True, cs=False, device=0):
    """write_sam_pairs() with the mates that mate rescue placed printed as mapped: the same device calls, texts and arguments, and
    rescue: the MateRescue of index.map_pairs_rescued over this Mapping and PairSelect.  A read with rescue.edits >= 0 that has no
    representative of its own, next to a mate that has one, gives one line: FLAG 0x1, 0x40 / 0x80, 0x10 from rescue.rev, 0x20 from
    the partner's strand and 0x2 -- on BOTH mates: a rescued pair is concordant by construction --; RNAME and POS = rescue.rs,
    target-local and 1-based; the CIGAR of its row (=, X, I, D: end to end); SEQ and QUAL oriented by oriented_rows; NM:i = edits,
    tp:A:R, MD:Z / cs:Z from record_diffs over the rescue's columns; RNEXT / PNEXT = the partner's place and TLEN by the
    template-length rule of kh_pair_chains over the two intervals.  The partner's line is updated to match: no 0x8, 0x20 from
    rescue.rev, 0x2, RNEXT / PNEXT = the rescued place, the same TLEN with the other sign.
    MAPQ of a rescued mate: pairs.mapq[partner] if rescue.span <= rescue.edits -- the end columns tied for the least distance are
    then one placement with its gaps shifted --, else 0: a second placement lies inside the window.
    A request that came back RESCUE_NONE or RESCUE_OVER, or with an alignment that faces no reference base (re == rs: a mate of at most
    max_edits bases against an empty window, all insertions), leaves the read as write_sam_pairs() prints it.
    -> (alignment lines written, rows skipped, unmapped reads)"""
    if pairs is None or rescue is None:
        raise ValueError("write_sam_rescued() needs a PairSelect and a MateRescue; write_sam_pairs() writes pairs without rescue")
    return _write_sam(fh, mapping, seq, ref_text, read_names, read_starts, read_ends, qual, ref_name, ref_len, ref_start, ref_base, targets, kept_only, unmapped, header, md, cs,
                      device, pairs, rescue)


def _write_sam(fh, mapping, seq, ref_text, read_names, read_starts, read_ends, qual, ref_name, ref_len, ref_start, ref_base, targets, kept_only, unmapped, header, md, cs,
               device, pairs, rescue=None):
    """the body of write_sam() (pairs None), write_sam_pairs() and write_sam_rescued()"""
    sb = _Buf.text(seq)
    seq = sb.obj
    layout = ReadLayout(read_starts, read_ends, sb.n, 1)
    layout.bounded(every=True)
    rs_, re_ = layout.host
    hm = _host_columns(mapping, parent=pairs is not None)
    n_reads = len(hm.select.best)
    if rs_.size != n_reads:
        raise ValueError("read_starts holds %d reads, the Mapping %d" % (rs_.size, n_reads))
    seg = hm.table.seg.astype(np.int64)
    if len(seg) and int(seg.max()) >= n_reads:
        raise ValueError("the table names read %d, the Mapping holds %d reads" % (int(seg.max()), n_reads))
    lo, hi = chain_read_intervals(NUMPY, layout, seg)
    place = namespace_of(seq).place      # a host column to where the texts live
    rec = mapping.records
    toff, ctext = cigar_text(rec.offsets, rec.ops, device)
    dlo, dhi = place(lo), place(hi)
    diffs = {kind: record_diffs(seq, ref_text, rec, mapping.table.rev, dlo, dhi, kind, ref_base, device) if want else None for kind, want in (("md", md), ("cs", cs))}
    # SEQ and QUAL: the oriented read for the primary rows that are printed, the read as given for the unmapped reads
    printable, _, _ = printable_rows(NUMPY, hm, targets, kept_only)
    mapped = _mapped_reads(hm, printable)
    need = printable & ((hm.select.flag & FLAG_PRIMARY) != 0) & mapped[seg] if len(seg) else np.zeros(0, dtype=bool)
    if pairs is not None:      # SEQ goes to the representatives and the 0x800 rows; the unmapped reads are those without a representative
        if n_reads % 2 or len(pairs.row) != n_reads:
            raise ValueError("pairs must hold one entry per read of the Mapping and the reads must come in pairs")
        pairs = pairs._replace(row=_host(pairs.row, np.int32), mapq=_host(pairs.mapq, np.uint8), tlen=_host(pairs.tlen, np.int32), flag=_host(pairs.flag, np.uint8))
        rep, role = _pair_roles(hm, pairs, printable)
        need, mapped = (role == ROLE_REP) | (role == ROLE_SUPP), rep >= 0
    show = ~mapped if unmapped else np.zeros(n_reads, dtype=bool)
    read_rev, rescued = np.zeros(n_reads, dtype=np.uint8), None
    if rescue is not None:      # the rescued reads: one CIGAR text and one difference string per request, SEQ oriented by rescue.rev
        rd, ed = _host(rescue.read, np.uint32).astype(np.int64), _host(rescue.edits, np.int32)
        r_rs, r_re, r_span = (_host(x, np.uint32).astype(np.int64) for x in (rescue.rs, rescue.re, rescue.span))
        r_rev = _host(rescue.rev, np.uint8) & 1
        inside = (rd >= 0) & (rd < n_reads)
        at = np.where(inside, rd, 0)
        take = inside & (ed >= 0) & (r_re > r_rs) & (rep[at] < 0) & (rep[at ^ 1] >= 0) if n_reads else np.zeros(len(rd), dtype=bool)      # (re == rs: a row of insertions only has no place)
        r_tgt = None
        if targets is not None:      # printable under the rule of the rows: inside one target
            inside, r_tgt = inside_target(NUMPY, targets, r_rs, r_re)
            take = take & inside
        coff, craw = _rows_of(cigar_text(rescue.offsets, rescue.ops, device))
        as_rec = ChainRecords(place(take.astype(np.uint8)), None, None, rescue.rs, rescue.re, None, None, None, None, rescue.offsets, rescue.ops)
        r_lo, r_hi = place(rs_[at].astype(np.uint32)), place(re_[at].astype(np.uint32))
        r_diffs = [(tag, _host(d.ok, np.uint8), *_rows_of((d.offsets, d.text))) for tag, d in
                   ((tag, record_diffs(seq, ref_text, as_rec, rescue.rev, r_lo, r_hi, kind, ref_base, device)) for tag, kind, want in (("MD", "md", md), ("cs", "cs", cs)) if want)]
        rescued = {}
        for j in np.flatnonzero(take):
            sr, tn = int(rd[j]), 0 if r_tgt is None else int(r_tgt[j])
            tname, t0 = (str(ref_name), int(ref_start)) if targets is None else (targets.names[tn], int(targets.starts[tn]))
            for tag, ok, _, _ in r_diffs:
                if not ok[j]:
                    raise ValueError("rescue request %d does not walk the two texts: pass the texts the MateRescue was made from" % j)
            rescued[sr] = dict(tn=tn, tname=tname, pos=int(r_rs[j]) - t0 + 1, rs=int(r_rs[j]), re=int(r_re[j]), rev=int(r_rev[j]), nm=int(ed[j]),
                               mapq=int(pairs.mapq[sr ^ 1]) if r_span[j] <= ed[j] else 0, cigar=craw[coff[j]:coff[j + 1]],
                               tags=["%s:Z:%s" % (tag, draw[doff[j]:doff[j + 1]]) for tag, _, doff, draw in r_diffs])
            show[sr], read_rev[sr] = True, r_rev[j]
    all_lo = np.concatenate([lo, rs_.astype(np.uint32)])
    all_hi = np.concatenate([np.where(need, hi, lo), np.where(show, re_, rs_).astype(np.uint32)]).astype(np.uint32)
    all_rev = np.concatenate([hm.table.rev & 1, read_rev]).astype(np.uint8)
    plo, phi, prev = place(all_lo), place(all_hi), place(all_rev)
    seq_rows = oriented_rows(seq, plo, phi, prev, True, device)
    qual_rows = oriented_rows(qual, plo, phi, prev, False, device) if qual is not None else None
    lines, skipped, n_unmapped = _sam_lines(hm, toff, ctext, seq_rows, read_names, qual_rows, diffs["md"], diffs["cs"], ref_name, ref_len, ref_start, targets,
                                            kept_only, unmapped, header, pairs, rescued)
    for ln in lines:
        fh.write(ln + "\n")
    n_head = len(sam_header(targets, ref_name, ref_len).splitlines()) if header else 0
    return len(lines) - n_head - (n_unmapped if unmapped else 0), skipped, n_unmapped


# ---- SAM lines on the device: the columns of every line from the Mapping (array glue), the text from kh_sam_lines
TAG_BASE, TAG_S2, TAG_MD, TAG_CS = 1, 2, 4, 8      # KH_SAMTAG_*
RNEXT_SAME = -2                                    # KH_SAM_RNEXT_SAME
LINE_COLUMNS = ("name", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual", "tags", "nm", "tp", "cm", "s1", "s2", "md", "cs")
LINE_DTYPES = (np.int32, np.uint32, np.int32, np.uint32, np.uint8, np.int32, np.int32, np.uint32, np.int32, np.int32, np.int32, np.uint8, np.uint32, np.uint8, np.uint32,
               np.int32, np.int32, np.int32, np.int32)
LineColumns = collections.namedtuple("LineColumns", LINE_COLUMNS + ("need", "show", "lines", "skipped", "unmapped_reads"))
SamText = collections.namedtuple("SamText", "header offsets text lines skipped unmapped_reads")


def names_csr(names):
    """a list of names -> (offsets uint64 [n + 1], bytes uint8) on the host: one join, one encode.  Names must be ASCII
    (UnicodeEncodeError otherwise): a character is then a byte and the lengths of the strings are the lengths of the rows."""
    names = [n if isinstance(n, str) else str(n) for n in names]
    offs = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=len(names)), out=offs[1:])
    return offs, np.frombuffer("".join(names).encode("ascii"), dtype=np.uint8)


def _is_csr(x):
    return isinstance(x, tuple) and len(x) == 2 and not isinstance(x[0], (str, bytes))


def sam_line_columns(xp, mapping, targets=None, ref_start=0, kept_only=True, unmapped=True, md=True, cs=False, pairs=None, diff_ok=(), refuse=()):
    """which rows and reads of a Mapping give a SAM line, in which order and with which columns: the rules of sam_lines() (and, with
    pairs, of write_sam_pairs() without rescued mates) restated as array operations over the namespace xp (kmerhash_amd._xp) in which
    the Mapping's columns -- and those of pairs, a PairSelect -- live: numpy, or torch on the Mapping's device.
    The rows the columns name: `name` read s of the read names; `rname` / `rnext` the target number (0 without targets; -1 '*';
    RNEXT_SAME '='); `cigar`, `md`, `cs` table row c; `seq` / `qual` row c of a CSR of n_rows + n_reads rows for a line of table row c
    that prints its bases, row n_rows + s for the line of unmapped read s, -1 for '*' (the layout sam_lines() takes).
    Order: reads ascending, a read's printable rows in table order, an unmapped read's line in the read's place -- table.seg does not
    descend (mapper.seg_offsets), so a line's number is two prefix sums and one searchsorted away; nothing is sorted.
    diff_ok: the ok columns of the RecordDiffs that will be printed; a printed row that is not ok raises the ValueError of write_sam.
    refuse: checks of the caller that ride along in the one read, as pairs (a 0-d count, a message): a count that is not zero raises
    ValueError(message), before the glue's own refusals.
    A ref_start beyond the start of a printed row is refused (ValueError): POS is an unsigned column, where sam_lines() prints a
    negative number.
    -> LineColumns: the nineteen columns of kh_sam_lines in its containers; need [n_rows] / show [n_reads] (bool): the table rows and
    the reads whose SEQ a line prints; lines, skipped, unmapped_reads: the triple of write_sam.  All numbers the host needs -- the
    three counts, the number of lines, the diff_ok check and the range check of table.seg -- are read together, once: with torch one
    wait for the stream."""
    t, sel, rec = mapping.table, mapping.select, mapping.records
    flag, rev = xp.signed(xp.col(sel.flag, np.uint8)), xp.signed(xp.col(t.rev, np.uint8)) & 1
    seg = xp.widen(xp.col(t.seg, np.uint32))
    n_rows, n_reads = len(flag), len(sel.best)
    if n_reads == 0 and n_rows:
        raise ValueError("the table names read %d, the Mapping holds %d reads" % (0, 0))
    printable, considered, tgt = printable_rows(xp, mapping, targets, kept_only)
    c, s = xp.arange(n_rows), xp.arange(n_reads)
    in_range = seg < n_reads
    segc = xp.minimum(seg, max(n_reads - 1, 0))      # (a row that names no read is reported below; until then it must address nothing)
    row_of = lambda col, at: col[at] if n_rows else xp.full(len(at), 0)      # noqa: E731  (a gather from the rows, which may be none)
    rs = xp.widen(xp.col(rec.rs, np.uint32))
    if targets is None:
        tn, pos = xp.full(n_rows, 0), rs - int(ref_start) + 1
    else:
        if int(ref_start) != 0:
            raise ValueError("with targets the starts are theirs: ref_start must be 0")
        tn = tgt
        pos = rs - targets.bound(xp, 0)[xp.maximum(tgt, 0)] + 1
    pri = (flag & FLAG_PRIMARY) != 0
    if pairs is None:
        best = xp.signed(xp.col(sel.best, np.int32))
        inside = (best >= 0) & (best < n_rows)
        mapped = inside & (row_of(xp.signed(printable), xp.where(inside, best, xp.full(n_reads, 0))) != 0)
        shown = printable & in_range & mapped[segc] if n_reads else printable & in_range
        r_flag = rev * 0x10 + xp.signed(~pri) * 0x100 + xp.signed(pri & (c != (best[segc] if n_reads else c))) * 0x800
        r_mapq = xp.signed(xp.col(sel.mapq, np.uint8))
        r_rnext, r_pnext, r_tlen = xp.full(n_rows, -1), xp.full(n_rows, 0), xp.full(n_rows, 0)
        u_flag, u_rname, u_pos, u_rnext = xp.full(n_reads, 4), xp.full(n_reads, -1), xp.full(n_reads, 0), xp.full(n_reads, -1)
    else:
        prow, pmapq, ptlen = xp.signed(xp.col(pairs.row, np.int32)), xp.signed(xp.col(pairs.mapq, np.uint8)), xp.signed(xp.col(pairs.tlen, np.int32))
        pflag = xp.signed(xp.col(pairs.flag, np.uint8))
        if n_reads % 2 or len(prow) != n_reads or len(pmapq) != n_reads or len(ptlen) != n_reads or len(pflag) != n_reads // 2:
            raise ValueError("pairs must hold one entry per read of the Mapping (row, mapq, tlen) and one per pair (flag), and the reads must come in pairs")
        parent = xp.signed(xp.col(sel.parent, np.int32))
        inside = (prow >= 0) & (prow < n_rows)
        at = xp.where(inside, prow, xp.full(n_reads, 0))
        rep = xp.where(inside & (row_of(xp.signed(printable), at) != 0) & (row_of(seg, at) == s), prow, xp.full(n_reads, -1))      # the row that represents a read
        mapped = rep >= 0
        own = xp.where(in_range, rep[segc], xp.full(n_rows, -1)) if n_reads else xp.full(n_rows, -1)
        shown = printable & (own >= 0)
        is_rep = c == own
        pri = ~(((flag & FLAG_PRIMARY) == 0) | (c == row_of(parent, xp.maximum(own, 0)))) | is_rep      # (ROLE_REP and ROLE_SUPP print bases; ROLE_SEC does not)
        mate = s ^ 1
        mr = rep[mate] if n_reads else rep
        mrc = xp.maximum(mr, 0)
        fl0 = 0x1 + xp.where((s & 1) != 0, xp.full(n_reads, 0x80), xp.full(n_reads, 0x40)) + xp.where(mr < 0, xp.full(n_reads, 0x8), row_of(rev, mrc) * 0x20)
        at = xp.where(mr >= 0, mr, rep)      # (an unmapped mate is placed at this read's representative: the mate columns point there)
        atc = xp.maximum(at, 0)
        mt = xp.where(at >= 0, row_of(tn, atc), xp.full(n_reads, -1))
        mpos = xp.where(at >= 0, row_of(pos, atc), xp.full(n_reads, 0))
        both = (rep >= 0) & (mr >= 0)
        proper = both & ((pflag[s >> 1] & 1) != 0) if n_reads else both      # (0x2 and TLEN need both representatives)
        g = lambda col: col[segc] if n_reads else xp.full(n_rows, 0)      # noqa: E731  (a per-read column at every row)
        r_flag = g(fl0) + rev * 0x10 + xp.signed(~is_rep & pri) * 0x800 + xp.signed(~pri) * 0x100 + xp.signed(is_rep & (g(xp.signed(proper)) != 0)) * 0x2
        r_mapq = xp.where(is_rep, g(pmapq), xp.signed(xp.col(sel.mapq, np.uint8)))
        r_rnext = xp.where(g(mt) == tn, xp.full(n_rows, RNEXT_SAME), g(mt))
        r_pnext = g(mpos)
        r_tlen = xp.where(is_rep & (g(xp.signed(both)) != 0), g(ptlen), xp.full(n_rows, 0))
        u_flag, u_rname, u_pos = fl0 + 0x4, mt, mpos
        u_rnext = xp.where(mr >= 0, xp.full(n_reads, RNEXT_SAME), xp.full(n_reads, -1))
    un_line = ~mapped if unmapped else (s < 0)
    need = shown & pri
    # the numbers the host must see, read once
    bad = None
    for ok in diff_ok:
        b = shown & (xp.signed(xp.col(ok, np.uint8)) == 0)
        bad = b if bad is None else bad | b
    numbers = [shown.sum(), un_line.sum(), (considered & in_range & ~shown).sum(), (~mapped).sum(), (shown & (pos < 0)).sum()]
    if n_rows:      # (a minimum or maximum needs an entry)
        numbers += [seg.max(), xp.where(bad, c, xp.full(n_rows, n_rows)).min() if bad is not None else seg.max() * 0 + n_rows]
    got = xp.ints([count for count, _ in refuse] + numbers)
    for count, (_, message) in zip(got, refuse):
        if count:
            raise ValueError(message)
    got = got[len(refuse):]
    n_shown, n_un, skipped, n_unmapped, neg_pos, seg_max, first_bad = (got + [0, 0])[:7]
    if n_rows and seg_max >= n_reads:
        raise ValueError("the table names read %d, the Mapping holds %d reads" % (seg_max, n_reads))
    if first_bad < n_rows:
        raise ValueError("row %d does not walk the two texts: make the Mapping with ref_order=True and pass the texts it was made from" % first_bad)
    if neg_pos:
        raise ValueError("ref_start lies beyond the start of %d rows: a position is printed as an unsigned number" % neg_pos)
    # the number of every line: shown rows before it plus unmapped-read lines before it
    rows_before, reads_before = xp.prefix(shown), xp.prefix(un_line)
    n_lines = n_shown + n_un
    line_of_row = rows_before[:-1] + (reads_before[segc] if n_reads else 0)
    line_of_read = reads_before[:-1] + rows_before[xp.searchsorted(seg, s)]
    src = xp.full(n_lines + 1, 0)      # line -> table row c, or n_rows + s; the last entry takes what gives no line
    src[xp.where(shown, line_of_row, xp.full(n_rows, n_lines))] = c
    src[xp.where(un_line, line_of_read, xp.full(n_reads, n_lines))] = n_rows + s
    src = src[:n_lines]
    is_row = src < n_rows
    cc = xp.where(is_row, src, xp.full(n_lines, 0))
    ss = xp.where(is_row, row_of(segc, cc), src - n_rows)
    R = lambda col: row_of(col, cc)      # noqa: E731
    U = lambda col: col[ss] if n_reads else xp.full(n_lines, 0)      # noqa: E731
    pick = lambda r, u: xp.where(is_row, r, u)      # noqa: E731
    zero, minus = xp.full(n_lines, 0), xp.full(n_lines, -1)
    lpri = R(xp.signed(pri)) != 0
    tags = xp.where(is_row, TAG_BASE + xp.signed(lpri) * TAG_S2 + (TAG_MD if md else 0) + (TAG_CS if cs else 0), zero)
    text_row = pick(xp.where(lpri, cc, minus), n_rows + ss)
    cols = dict(name=ss, flag=pick(R(r_flag), U(u_flag)), rname=pick(R(tn), U(u_rname)), pos=pick(R(pos), U(u_pos)), mapq=pick(R(r_mapq), zero), cigar=pick(cc, minus),
                rnext=pick(R(r_rnext), U(u_rnext)), pnext=pick(R(r_pnext), U(u_pos)), tlen=pick(R(r_tlen), zero), seq=text_row, qual=text_row, tags=tags,
                nm=pick(R(xp.widen(xp.col(rec.nm, np.uint32))), zero), tp=xp.where(lpri, xp.full(n_lines, ord("P")), xp.full(n_lines, ord("S"))),
                cm=pick(R(xp.widen(xp.col(t.count, np.uint32))), zero), s1=pick(R(xp.signed(xp.col(t.score, np.int32))), zero),
                s2=pick(R(xp.signed(xp.col(sel.sub, np.int32))), zero), md=pick(cc, minus), cs=pick(cc, minus))
    return LineColumns(*(xp.narrow(cols[k], dt) for k, dt in zip(LINE_COLUMNS, LINE_DTYPES)), need, un_line, n_shown, skipped, n_unmapped)


def _csr_where(names, xp, what):
    """read or target names -> (offsets _Buf, bytes _Buf): a list goes through names_csr() and to where the Mapping lives; a ready
    (offsets, bytes) CSR must live there already"""
    offs, text = names if _is_csr(names) else (xp.place(a) for a in names_csr(names))
    ob, tb = _Buf(offs, np.uint64), _Buf.text(text)
    if ob.n < 1:
        raise ValueError("the offsets of %s must hold one entry per name and one more" % what)
    return ob, tb


def sam_lines_text(names, tnames, cigar, seq, qual, md, cs, columns, device=0):
    """kh_sam_lines: SAM lines from line columns (the definition is in include/kmerhash_amd.h).  names, tnames, cigar, seq, qual, md,
    cs: byte CSRs (offsets, text), each or None for an absent one; columns: the nineteen line columns in the order of LINE_COLUMNS.
    -> (offsets, text): line i is text[offsets[i]:offsets[i + 1]], its line feed included.  numpy in, numpy out (uint64, uint8); CUDA
    tensors in, tensors out on the current stream (int64, uint8); count, then emit, one wait per pass."""
    cb = [_Buf(x, dt) for x, dt in zip(columns, LINE_DTYPES)]
    check_same("the line columns must live in the same memory and have one entry per line", *cb)
    like, n_lines, args = cb[0], cb[0].n, []
    for pair in (names, tnames, cigar, seq, qual, md, cs):
        if pair is None:
            args += [None, None, 0, 0]
            continue
        ob, tb = (_Buf(pair[0], np.uint64), _Buf.text(pair[1])) if not isinstance(pair[0], _Buf) else pair
        check_same("the CSRs and the line columns must live in the same memory", like, ob, tb, length=False)
        if ob.n < 1:
            raise ValueError("the offsets of a CSR hold one entry per row and one more")
        args += [ob.ptr if ob.n > 1 else None, tb.ptr_or_null, ob.n - 1, tb.n]
    if n_lines > 2 ** 31:
        raise ValueError("at most 2^31 lines per call, got %d" % n_lines)
    offs, optr = alloc(like, n_lines + 1, np.uint64, zero=True)
    if n_lines == 0:
        return offs, alloc(like, 0, np.uint8)[0]
    lead = (*args, *(b.ptr for b in cb), n_lines, like.where, optr)
    return offs, two_pass("kh_sam_lines", lead, like, np.uint8, device)


def sam_text(mapping, seq, ref_text, read_names, read_starts, read_ends=None, qual=None, ref_name=None, ref_len=None, ref_start=0, ref_base=0, targets=None,
             kept_only=True, unmapped=True, md=True, cs=False, pairs=None, device=0):
    """the rows of a Mapping as the text of a SAM file, assembled where the Mapping lives: the file write_sam() writes -- with pairs (a
    PairSelect) the file write_sam_pairs() writes -- byte for byte, without a line ever being formatted on the host.  Arguments as
    write_sam(); read_names (and the names of targets) may be a ready (offsets, bytes) CSR that lives where the Mapping lives instead
    of a list of ASCII names (names_csr() makes one).
    Device calls: cigar_text(), record_diffs() per difference string asked for, oriented_rows() for SEQ and for QUAL over the rows and
    the reads (the layout of sam_lines()), the array glue sam_line_columns() and kh_sam_lines.  No loop over rows or reads runs in
    Python and SEQ, QUAL, the CIGAR text and the difference strings are never copied to the host; beyond the waits of those calls
    (one per pass of a count-then-emit call) there is one: the glue reads its counts and checks together, once -- the bounds check of
    read_starts / read_ends included where both are CUDA tensors (read_ends may be None); given on the host, or one of each, they
    are checked there before anything is queued, and a CUDA tensor among them then costs a copy and a wait of its own.
    One difference from write_sam(): a ref_start beyond the start of a printed row raises ValueError -- POS is an unsigned column of
    kh_sam_lines, where write_sam() prints a negative POS.
    A printed row whose difference string is not ok raises the ValueError of write_sam(): make the Mapping with ref_order=True.
    A MateRescue is not taken: write_sam_rescued() keeps the host path.
    -> SamText(header, offsets, text, lines, skipped, unmapped_reads): header the bytes of sam_header(); text the body, line i at
    text[offsets[i]:offsets[i + 1]] -- uint8 / uint64 numpy arrays for numpy input, uint8 / int64 tensors on the current stream for
    CUDA tensors; (lines, skipped, unmapped_reads) the triple write_sam() / write_sam_pairs() return."""
    head = sam_header(targets, ref_name, ref_len).encode()      # (checks ref_name / ref_len against targets)
    sb = _Buf.text(seq)
    seq = sb.obj
    xp = namespace_of(seq)
    layout = ReadLayout(read_starts, read_ends, sb.n, 1)
    on_device = lambda x: _is_tensor(x) and x.is_cuda      # noqa: E731
    late = not xp.host and on_device(read_starts) and (read_ends is None or on_device(read_ends))      # the layout lives on the device: its check rides in the glue's one read
    if not late:
        layout.bounded(every=True)
    rec, t = mapping.records, mapping.table
    n_reads = len(mapping.select.best)
    if layout.n_reads != n_reads:
        raise ValueError("read_starts holds %d reads, the Mapping %d" % (layout.n_reads, n_reads))
    names = _csr_where(read_names, xp, "read_names")
    if names[0].n != n_reads + 1:
        raise ValueError("read_names holds %d names, the Mapping %d reads" % (names[0].n - 1, n_reads))
    tnames = _csr_where(getattr(targets, "names_csr", None) or targets.names, xp, "the target names") if targets is not None else _csr_where([str(ref_name)], xp, "ref_name")
    starts, ends = layout.on(xp)
    bad_layout = "read_starts and read_ends must hold one byte offset per read, 0 <= read_starts[s] <= read_ends[s] <= len(seq)"
    if len(ends) != len(starts):
        raise ValueError(bad_layout)
    segc = xp.minimum(xp.widen(xp.col(t.seg, np.uint32)), max(n_reads - 1, 0))      # (a row that names no read: the glue refuses it below)
    lo, hi = (xp.narrow(col[segc] if n_reads else segc, np.uint32) for col in (starts, ends))
    ctext = cigar_text(rec.offsets, rec.ops, device)
    diffs = {kind: record_diffs(seq, ref_text, rec, t.rev, lo, hi, kind, ref_base, device) if want else None for kind, want in (("md", md), ("cs", cs))}
    L = sam_line_columns(xp, mapping, targets, ref_start, kept_only, unmapped, md, cs, pairs, [d.ok for d in diffs.values() if d is not None],
                         [(((ends < starts) | (ends > sb.n) | (starts < 0)).sum(), bad_layout)] if late else [])      # (the device calls before this clamp what
    #                          they are given: a wrong layout gave them wrong rows, never a stray access)
    # SEQ and QUAL: the oriented read for the rows that print their bases, the read as given for the unmapped reads
    all_lo = xp.narrow(xp.concat([xp.widen(lo), starts]), np.uint32)
    all_hi = xp.narrow(xp.concat([xp.where(L.need, xp.widen(hi), xp.widen(lo)), xp.where(L.show, ends, starts)]), np.uint32)
    all_rev = xp.narrow(xp.concat([xp.signed(xp.col(t.rev, np.uint8)) & 1, xp.full(n_reads, 0)]), np.uint8)
    seq_rows = oriented_rows(seq, all_lo, all_hi, all_rev, True, device)
    qual_rows = oriented_rows(qual, all_lo, all_hi, all_rev, False, device) if qual is not None else None
    offs, text = sam_lines_text(names, tnames, ctext, seq_rows, qual_rows, *((d.offsets, d.text) if d is not None else None for d in (diffs["md"], diffs["cs"])),
                                L[:len(LINE_COLUMNS)], device)
    return SamText(head, offs, text, L.lines, L.skipped, L.unmapped_reads)


def write_sam_bytes(fh, mapping, seq, ref_text, read_names, read_starts, read_ends=None, qual=None, ref_name=None, ref_len=None, ref_start=0, ref_base=0, targets=None,
                    kept_only=True, unmapped=True, header=True, md=True, cs=False, pairs=None, device=0):
    """write_sam() -- with pairs (a PairSelect) write_sam_pairs() -- into the BINARY file `fh`, the lines assembled on the device
    (sam_text(), which lists the device calls): the header when `header`, then the body, which comes to the host as one copy of the
    finished text.  The bytes are those the host writers give, encoded -- but a ref_start beyond the start of a printed
    row, for which write_sam() prints a negative POS, raises ValueError here.  A MateRescue is not taken: write_sam_rescued() keeps the
    host path.
    -> (alignment lines written, rows skipped, unmapped reads)"""
    st = sam_text(mapping, seq, ref_text, read_names, read_starts, read_ends, qual, ref_name, ref_len, ref_start, ref_base, targets, kept_only, unmapped, md, cs, pairs,
                  device)
    if header:
        fh.write(st.header)
    fh.write(_host(st.text, np.uint8).tobytes())
    return st.lines, st.skipped, st.unmapped_reads
