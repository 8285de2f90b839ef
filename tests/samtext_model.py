"""TEST HELPER (not collected): kh_sam_lines on Python integers and bytes -- the definition of include/kmerhash_amd.h restated: line
columns and byte CSRs to the text of SAM alignment lines.  A CSR is (offsets, text) with text as bytes, or None for an absent one; the
line columns are the keyword arguments of sam_lines(), each one value per line."""

TAG_BASE, TAG_S2, TAG_MD, TAG_CS = 1, 2, 4, 8      # KH_SAMTAG_*
RNEXT_SAME = -2                                    # KH_SAM_RNEXT_SAME
COLUMNS = ("name", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual", "tags", "nm", "tp", "cm", "s1", "s2", "md", "cs")


def decimal(v):
    """what "%d" prints, digit by digit (the tests hold it against "%d")"""
    v = int(v)
    mag, digits = abs(v), []
    while True:
        digits.append(48 + mag % 10)
        mag //= 10
        if mag == 0:
            break
    return (b"-" if v < 0 else b"") + bytes(reversed(digits))


def row(csr, r):
    """-> (inside, bytes): the row clamped to the text; outside: no CSR, or r not in [0, rows)"""
    if csr is None:
        return False, b""
    offsets, text = csr
    text = bytes(text)
    if not 0 <= int(r) < len(offsets) - 1:
        return False, b""
    a, b = min(int(offsets[r]), len(text)), min(int(offsets[r + 1]), len(text))
    return True, text[a:b] if b > a else b""


def name_field(csr, r):
    inside, b = row(csr, r)
    return b if inside else b"*"


def seq_field(csr, r):
    return row(csr, r)[1] or b"*"


def line(names, tnames, cigar, seq, qual, md, cs, name, flag, rname, pos, mapq, cigar_row, rnext, pnext, tlen, seq_row, qual_row, tags, nm, tp, cm, s1, s2, md_row,
         cs_row):
    f = [name_field(names, name), decimal(flag), name_field(tnames, rname), decimal(pos), decimal(mapq), name_field(cigar, cigar_row),
         b"=" if int(rnext) == RNEXT_SAME else name_field(tnames, rnext), decimal(pnext), decimal(tlen), seq_field(seq, seq_row), seq_field(qual, qual_row)]
    if tags & TAG_BASE:
        f += [b"NM:i:" + decimal(nm), b"tp:A:" + bytes([int(tp)]), b"cm:i:" + decimal(cm), b"s1:i:" + decimal(s1)]
    if tags & TAG_S2:
        f.append(b"s2:i:" + decimal(s2))
    if tags & TAG_MD:
        f.append(b"MD:Z:" + row(md, md_row)[1])
    if tags & TAG_CS:
        f.append(b"cs:Z:" + row(cs, cs_row)[1])
    return b"\t".join(f) + b"\n"


def sam_lines(names, tnames, cigar, seq, qual, md, cs, cols):
    """cols: {column name: one value per line} with the names of COLUMNS -> (offsets, text)"""
    n = len(cols["name"])
    assert sorted(cols) == sorted(COLUMNS) and all(len(cols[c]) == n for c in COLUMNS)
    offsets, out = [0], []
    for i in range(n):
        c = {k: int(cols[k][i]) for k in COLUMNS}
        out.append(line(names, tnames, cigar, seq, qual, md, cs, c["name"], c["flag"], c["rname"], c["pos"], c["mapq"], c["cigar"], c["rnext"], c["pnext"], c["tlen"],
                        c["seq"], c["qual"], c["tags"], c["nm"], c["tp"], c["cm"], c["s1"], c["s2"], c["md"], c["cs"]))
        offsets.append(offsets[-1] + len(out[-1]))
    return offsets, b"".join(out)
