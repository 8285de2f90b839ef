"""TEST HELPER (not collected): the definitions of kh_fastq_records and kh_pack_rows (include/kmerhash_amd.h) as Python loops over
bytes, and read_fastq() stated over them.  Plain ints and bytes; no numpy in the rules themselves."""

STRIP_MATE = 1
NO_AT, NO_PLUS, LENGTHS, NO_NAME = 1, 2, 4, 8


def lines_of(text):
    """[(start, end)] of every line: line j runs from after newline j - 1 up to, not including, newline j; a non-empty remainder after
    the last newline is a last line; one '\\r' directly before the end of a line is not part of it"""
    out, start = [], 0
    for i in range(len(text)):
        if text[i] == 10:
            out.append((start, i))
            start = i + 1
    if start < len(text):
        out.append((start, len(text)))
    return [(a, b - 1 if b > a and text[b - 1] == 13 else b) for a, b in out]


def fastq_records(text, flags=0):
    """-> (rows, n_bad, tail_lines): rows[r] = (name_lo, name_hi, seq_lo, seq_hi, qual_lo, status)"""
    text = bytes(text)
    lines = lines_of(text)
    n_rec = len(lines) // 4
    rows, n_bad = [], 0
    for r in range(n_rec):
        (h0, h1), (s0, s1), (p0, p1), (q0, q1) = lines[4 * r:4 * r + 4]
        status = 0
        at = h1 > h0 and text[h0] == ord("@")
        if not at:
            status |= NO_AT
        if not (p1 > p0 and text[p0] == ord("+")):
            status |= NO_PLUS
        if q1 - q0 != s1 - s0:
            status |= LENGTHS
        name_lo = h0 + (1 if at else 0)
        name_hi = name_lo
        while name_hi < h1 and text[name_hi] > 0x20:
            name_hi += 1
        if (flags & STRIP_MATE) and name_hi - name_lo > 2 and text[name_hi - 2:name_hi] in (b"/1", b"/2"):
            name_hi -= 2
        if name_hi == name_lo:
            status |= NO_NAME
        if status:
            s1, q0 = s0, s0
            n_bad += 1
        rows.append((name_lo, name_hi, s0, s1, q0, status))
    tail = sum(1 for a, b in lines[4 * n_rec:] if b > a)
    return rows, n_bad, tail


def pack_rows(text, lo, hi, dst, sep, out):
    """out: a bytearray, written in place and returned"""
    n, out_n = len(text), len(out)
    for a, b, d in zip(lo, hi, dst):
        length = b - a if a <= b <= n else 0
        for j in range(length):
            if d + j < out_n:
                out[d + j] = text[a + j]
        if sep >= 0 and d + length < out_n:
            out[d + length] = sep
    return out


def read_fastq(texts, strip_mate=None):
    """strict=False of kmerhash_amd.read_fastq over one or two texts -> dict(seq, qual, read_starts, read_ends, names (offsets, bytes),
    n_reads, status, n_bad, tail_lines, counts)"""
    flags = STRIP_MATE if (len(texts) == 2 if strip_mate is None else strip_mate) else 0
    per = [fastq_records(t, flags) for t in texts]
    n_pairs = max(len(p[0]) for p in per)
    seq, qual, names, starts, ends, noff, status = bytearray(), bytearray(), bytearray(), [], [], [0], []
    for p in range(n_pairs):
        for t, (rows, _, _) in zip(texts, per):
            name_lo, name_hi, s0, s1, q0, st = rows[p] if p < len(rows) else (0, 0, 0, 0, 0, 0)
            starts.append(len(seq))
            seq += bytes(t[s0:s1]) + b"\n"
            qual += bytes(t[q0:q0 + s1 - s0]) + b"\n"
            ends.append(len(seq) - 1)
            names += bytes(t[name_lo:name_hi])
            noff.append(len(names))
            status.append(st)
    return dict(seq=bytes(seq), qual=bytes(qual), read_starts=starts, read_ends=ends, names=(noff, bytes(names)), n_reads=len(starts), status=status,
                n_bad=[p[1] for p in per], tail_lines=[p[2] for p in per], counts=[len(p[0]) for p in per])
