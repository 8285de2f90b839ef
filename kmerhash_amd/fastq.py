"""FASTQ in: the input side of the mapper.  kh_fastq_records finds the records of a FASTQ text -- where the name, the bases and the
qualities of every read are -- and kh_pack_rows gathers byte rows to given places (include/kmerhash_amd.h holds both definitions,
tests/fastq_model.py the models); read_fastq() puts them together into what the mapper calls and the SAM writers take: the reads joined
by line feeds, the qualities in the same layout, read_starts / read_ends and a names CSR, all where the text lives.  No loop over reads
runs in Python and no read, quality string or name is copied to the host."""
import collections
import ctypes as C

import numpy as np

from . import _capi as K
from ._call import _Buf, alloc, check, check_same, stream_of
from ._xp import namespace_of

FastqRecords = collections.namedtuple("FastqRecords", "name_lo name_hi seq_lo seq_hi qual_lo status n_bad tail_lines")
Reads = collections.namedtuple("Reads", "seq qual read_starts read_ends names n_reads status")
STRIP_MATE = 1                                        # KH_FASTQ_STRIP_MATE
NO_AT, NO_PLUS, LENGTHS, NO_NAME = 1, 2, 4, 8         # KH_FASTQ_NO_AT ...: the bits of status
COLUMNS = ("name_lo", "name_hi", "seq_lo", "seq_hi", "qual_lo")


def fastq_records(text, strip_mate=False, device=0):
    """the record structure of a FASTQ text (kh_fastq_records): per record of four lines the byte offsets of its name [name_lo, name_hi)
    (behind the '@', up to the first blank; with strip_mate without a closing /1 or /2), of its bases [seq_lo, seq_hi) and of its
    qualities qual_lo, and status (0, or bits NO_AT, NO_PLUS, LENGTHS, NO_NAME: such a record is kept as an empty read).
    -> FastqRecords(name_lo, name_hi, seq_lo, seq_hi, qual_lo, status, n_bad, tail_lines): n_bad the records with a status, tail_lines
    the non-empty lines behind the last whole record.  bytes / numpy in, numpy out (uint32, uint8); a CUDA uint8 tensor in, tensors out
    on the current stream (int32 holding the uint32 bits, uint8); count, then emit, one wait per pass."""
    tb = _Buf.text(text)
    if tb.n >= 2 ** 32:
        raise ValueError("a text of less than 2^32 bytes per call, got %d" % tb.n)
    fn, stream = K.lib().kh_fastq_records, stream_of(tb, device)
    n_rec, n_bad, tail = C.c_uint64(), C.c_uint64(), C.c_uint32()
    lead = (tb.ptr_or_null, tb.n, STRIP_MATE if strip_mate else 0, tb.where)
    counts = (C.byref(n_rec), C.byref(n_bad), C.byref(tail), device, stream)
    check(fn(*lead, None, None, None, None, None, None, 0, *counts), "kh_fastq_records")
    cols = [alloc(tb, n_rec.value, np.uint32, empty=True) for _ in COLUMNS] + [alloc(tb, n_rec.value, np.uint8, empty=True)]
    if n_rec.value:
        check(fn(*lead, *(p for _, p in cols), n_rec.value, *counts), "kh_fastq_records")
    return FastqRecords(*(c for c, _ in cols), n_bad.value, tail.value)


def pack_rows(text, lo, hi, dst, out_len, sep=None, out=None, device=0):
    """byte rows gathered to given places (kh_pack_rows): out[dst[i] + j] = text[lo[i] + j] for j < hi[i] - lo[i] and, with sep (a byte
    value), out[dst[i] + hi[i] - lo[i]] = sep behind every row.  A row outside the text is empty; a store at or beyond out_len is
    dropped; bytes no row covers are not written; keeping the rows apart is the caller's.  out=None: out_len zeroed bytes where the
    text lives; a given out (a contiguous uint8 array or tensor of out_len bytes, where the text lives) is written in place -- that is
    how two files interleave into one buffer.  -> out.  Device memory: queued on the current stream, no wait."""
    tb, lb, hb, db = _Buf.text(text), _Buf(lo, np.uint32), _Buf(hi, np.uint32), _Buf(dst, np.uint64)
    out_len = int(out_len)
    if out is None:
        out, optr = alloc(tb, out_len, np.uint8, zero=True)
    else:
        ob = _Buf(out, np.uint8)
        if ob.obj is not out or ob.n != out_len or ob.where != tb.where:
            raise ValueError("out must be a contiguous uint8 array or tensor of out_len = %d bytes where the text lives" % out_len)
        optr = ob.ptr
    check_same("text, lo, hi and dst must live in the same memory", tb, lb, hb, db, length=False)
    check_same("lo, hi and dst must have one entry per row, got %d, %d and %d" % (lb.n, hb.n, db.n), lb, hb, db)
    if sep is not None and not 0 <= int(sep) <= 255:
        raise ValueError("sep must be None or a byte value, got %r" % (sep,))
    if tb.n >= 2 ** 32 or out_len >= 2 ** 32 or lb.n > 2 ** 31:
        raise ValueError("texts of less than 2^32 bytes and at most 2^31 rows per call")
    if lb.n and out_len:
        check(K.lib().kh_pack_rows(tb.ptr_or_null, tb.n, lb.ptr, hb.ptr, db.ptr, lb.n, -1 if sep is None else int(sep), tb.where, optr, out_len, device,
                                   stream_of(tb, device)), "kh_pack_rows")
    return out


STATUS_WORDS = ((NO_AT, "its first line does not begin with '@'"), (NO_PLUS, "its third line does not begin with '+'"),
                (LENGTHS, "its quality line is not as long as its sequence line"), (NO_NAME, "its name is empty"))


def read_fastq_glue(xp, texts, recs, strict, pack):
    """the array glue of read_fastq(), written once over the namespace xp (kmerhash_amd._xp) in which the texts and the columns live:
    texts: one or two FASTQ texts; recs: their FastqRecords; pack(text, lo, hi, dst, out_len, sep, out): pack_rows.  Lengths, their
    cumulative sums as destinations, the interleave of two files, the mate-name test; ONE read of the totals and checks together."""
    F = len(texts)
    counts = [len(r.status) for r in recs]
    if strict:      # what the counts of fastq_records say is known on the host already
        for f, r in enumerate(recs):
            if r.n_bad:
                st = xp.signed(xp.col(r.status, np.uint8))
                first, = xp.ints([xp.nonzero(st != 0)[0]])
                bits, = xp.ints([st[first]])
                raise ValueError("record %d of text %d is malformed: %s (strict=False keeps it as an empty read)" %
                                 (first, f + 1, "; ".join(w for b, w in STATUS_WORDS if bits & b)))
            if r.tail_lines:
                raise ValueError("text %d ends inside a record: %d lines follow its %d whole records" % (f + 1, r.tail_lines, counts[f]))
        if F == 2 and counts[0] != counts[1]:
            raise ValueError("the two texts hold %d and %d records: record %d has no mate" % (counts[0], counts[1], min(counts)))
    n_pairs = max(counts)
    n_reads = F * n_pairs

    def column(f, name, np_dtype=np.uint32):      # (a text with fewer records than its mate file, strict=False: empty reads without a name)
        x = xp.widen(xp.col(getattr(recs[f], name), np_dtype))
        return x if counts[f] == n_pairs else xp.concat([x, xp.full(n_pairs - counts[f], 0)])

    def weave(parts):      # record p of text f is read F * p + f
        if F == 1:
            return parts[0]
        out = xp.full(n_reads, 0)
        for f, p in enumerate(parts):
            out[f::F] = p
        return out

    col = [{name: column(f, name) for name in COLUMNS} for f in range(F)]
    slen = [c["seq_hi"] - c["seq_lo"] for c in col]
    nlen = [c["name_hi"] - c["name_lo"] for c in col]
    spre, npre = xp.prefix(weave(slen) + 1), xp.prefix(weave(nlen))      # every read is followed by one line feed
    checks = [spre[-1], npre[-1]]
    mates = strict and F == 2
    if mates:      # lengths against lengths, then the names of each text packed on their own against each other: equal lengths, equal places
        room = min(len(t) for t in texts)      # (the names of a text are fewer bytes than the text)
        own = [xp.prefix(l) for l in nlen]
        packed = [pack(texts[f], xp.narrow(col[f]["name_lo"], np.uint32), xp.narrow(col[f]["name_hi"], np.uint32), xp.narrow(own[f][:-1], np.uint64), room, None,
                       xp.full(room, 0, np.uint8)) for f in range(F)]
        checks += [(nlen[0] != nlen[1]).sum(), (packed[0] != packed[1]).sum()]
    nums = xp.ints(checks)
    if mates and (nums[2] or nums[3]):
        first = []
        if nums[2]:
            first += xp.ints([xp.nonzero(nlen[0] != nlen[1])[0]])
        if nums[3]:      # the first byte that differs lies in the name of the last record that starts at or before it
            first += xp.ints([xp.searchsorted(own[0][1:], xp.nonzero(packed[0] != packed[1])[:1], right=True)[0]])
        raise ValueError("record %d carries different names in the two texts (strip_mate=%s)" % (min(first), "True drops a closing /1 or /2"))
    total, ntotal = nums[0], nums[1]
    starts = spre[:-1]
    ends = starts + weave(slen)
    seq, qual, names = xp.full(total, 10, np.uint8), xp.full(total, 10, np.uint8), xp.full(ntotal, 0, np.uint8)
    for f in range(F):
        c, d = col[f], xp.narrow(starts[f::F], np.uint64)
        pack(texts[f], xp.narrow(c["seq_lo"], np.uint32), xp.narrow(c["seq_hi"], np.uint32), d, total, 10, seq)
        pack(texts[f], xp.narrow(c["qual_lo"], np.uint32), xp.narrow(c["qual_lo"] + slen[f], np.uint32), d, total, 10, qual)
        pack(texts[f], xp.narrow(c["name_lo"], np.uint32), xp.narrow(c["name_hi"], np.uint32), xp.narrow(npre[:-1][f::F], np.uint64), ntotal, None, names)
    status = xp.narrow(weave([column(f, "status", np.uint8) for f in range(F)]), np.uint8)
    return Reads(seq, qual, starts, ends, (xp.narrow(npre, np.uint64), names), n_reads, status)


def read_fastq(text, text2=None, strict=True, strip_mate=None, device=0):
    """a FASTQ text (bytes, a uint8 array, or a uint8 CUDA tensor) as the arguments of the mapper and of the SAM writers
    -> Reads(seq, qual, read_starts, read_ends, names, n_reads, status), everything where the text lives:
    seq: every read followed by one line feed -- read_starts[0] = 0, read_starts[s + 1] = read_ends[s] + 1; a line feed is no base, so
    no window, link or extension crosses a read; qual: the qualities in the same layout, qual[i] belongs to seq[i], as write_sam() asks;
    read_starts, read_ends: int64; names: an (offsets, bytes) CSR, what sam_text() and write_sam_bytes() take as read_names (uint64 /
    uint8 arrays, int64 / uint8 tensors); status: per read the status of fastq_records().
    text2: the second file of a paired run; the reads interleave -- record p of text is read 2p, record p of text2 read 2p + 1 -- as
    map_pairs() wants them, and strip_mate then defaults to True (a closing /1 or /2 is no part of a name).
    strict: ValueError -- its message names the first offending record -- for a malformed record, lines of a record cut short behind the
    last whole one, two texts with different record counts, and mates whose names differ.  strict=False: a malformed record stays in
    its place as an empty read (status says why), the shorter of two texts is filled up with empty reads, nothing else is checked.
    Device calls: fastq_records() per text, then pack_rows() per text for the bases, the qualities and the names.  Waits on a device
    text: those of fastq_records() (one per pass) and ONE read of the totals and the checks together."""
    bufs = [_Buf.text(t) for t in ((text,) if text2 is None else (text, text2))]
    check_same("the two texts must live in the same memory", *bufs, length=False)
    strip = (text2 is not None) if strip_mate is None else bool(strip_mate)
    texts = [b.obj for b in bufs]
    recs = [fastq_records(t, strip, device) for t in texts]
    return read_fastq_glue(namespace_of(texts[0]), texts, recs, bool(strict),
                           lambda t, lo, hi, dst, out_len, sep, out: pack_rows(t, lo, hi, dst, out_len, sep, out, device))
