"""GPU: ix.map, then write_sam, on both index classes, against one reference and against a contig table: the planted reads of
tests/test_gpu_records_index.py (substitutions, an insertion, a deletion, both strands, clipped ends, a read without a whole alignment, a
region that stands twice).  EVERY mapped line is checked on its own, from nothing but the line and the two texts: the CIGAR consumes
len(SEQ) read bases, SEQ is the read or its reverse complement and QUAL goes with it, the reference rebuilt from SEQ, CIGAR and MD and,
separately, from cs is the reference text under the line, NM is the edits MD and the CIGAR show.  The lines hold an X, an I and a D run,
a reverse-strand row, a soft clip, a secondary and an unmapped read; write_paf prints the same rows; a tensor Mapping gives the same file
as a numpy one."""
import io
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from edits_cases import revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402
from test_gpu_records_index import N_READS, REF_LEN, make_reads  # noqa: E402

CUT = 9000      # with targets the reference is two contigs: [0, CUT) and [CUT, REF_LEN)


def ref_from_md(seq, cigar, md):
    """the reference under an alignment, from the oriented read, its CIGAR and its MD"""
    m, qi = [], 0
    for n, o in cigar:
        if o in "SI":
            qi += n
        elif o in "=X":
            m += list(seq[qi:qi + n]); qi += n
        else:
            m += [None] * n
    assert qi == len(seq)
    at = 0
    for num, dele, sub in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            assert all(x is not None for x in m[at:at + int(num)])
            at += int(num)
        elif dele:
            assert m[at:at + len(dele)] == [None] * len(dele)
            m[at:at + len(dele)] = list(dele); at += len(dele)
        else:
            assert m[at] is not None and m[at] != sub
            m[at] = sub; at += 1
    assert at == len(m)
    return "".join(m)


def ref_from_cs(seq, cigar, cs):
    """the same from the oriented read and its short cs string alone (the CIGAR only says how much the head clips)"""
    qi = cigar[0][0] if cigar[0][1] == "S" else 0
    out = []
    for tok in re.findall(r":\d+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+", cs):
        if tok[0] == ":":
            out.append(seq[qi:qi + int(tok[1:])]); qi += int(tok[1:])
        elif tok[0] == "*":
            assert seq[qi] == tok[2].upper() != tok[1].upper()
            out.append(tok[1].upper()); qi += 1
        elif tok[0] == "+":
            assert seq[qi:qi + len(tok) - 1] == tok[1:].upper()
            qi += len(tok) - 1
        else:
            out.append(tok[1:].upper())
    assert qi + (cigar[-1][0] if cigar[-1][1] == "S" and len(cigar) > 1 else 0) == len(seq)
    return "".join(out)


@pytest.mark.parametrize("with_targets", [False, True])
@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 35)])
def test_every_line_of_the_sam_file(cls, k, with_targets):
    ref, seq, starts, ends_at = make_reads()
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], [ref[:CUT], ref[CUT:]]) if with_targets else None
    rt = T.text.copy() if with_targets else np.frombuffer(ref, dtype=np.uint8).copy()
    qt = np.frombuffer(seq, dtype=np.uint8).copy()
    qual = (33 + np.arange(len(qt)) % 41).astype(np.uint8)
    names = ["read%d" % i for i in range(N_READS)]
    where = dict(targets=T) if with_targets else dict(ref_name="ref", ref_len=REF_LEN)
    files = {}
    for dev in (False, True):
        mk = to_dev if dev else (lambda a: a)
        ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
        try:
            ix.build_sequences(mk(rt))
            mp = ix.map(mk(qt), mk(rt), read_starts=starts, read_ends=ends_at, min_score=20, min_count=2, pri_pct=50, targets=T)
            fh, ph = io.StringIO(), io.StringIO()
            counts = kh.write_sam(fh, mp, mk(qt), mk(rt), names, starts, ends_at, qual=mk(qual), md=True, cs=True, **where)
            paf = kh.write_paf(ph, mp, names, k=k, **where)
            files[dev] = (fh.getvalue(), counts, ph.getvalue(), paf)
        finally:
            ix.close()
    assert files[False] == files[True], "a tensor Mapping gives another file than a numpy one"
    text, (written, skipped, n_unmapped), paf_text, (paf_written, paf_skipped) = files[False]
    lines = text.splitlines()
    head = [l for l in lines if l.startswith("@")]
    assert head == kh.sam_header(**where).splitlines() and lines[:len(head)] == head
    body = [l.split("\t") for l in lines[len(head):]]
    mapped = [f for f in body if not int(f[1]) & 4]
    unmapped = [f for f in body if int(f[1]) & 4]
    assert (written, n_unmapped) == (len(mapped), len(unmapped))
    assert [int(f[0][4:]) for f in body] == sorted(int(f[0][4:]) for f in body), "reads ascend"
    assert len({f[0] for f in body}) == N_READS, "every read has a line"
    # write_paf prints the same rows, but for the printable rows of reads whose best row is not
    lost = {f[0] for f in unmapped}
    paf_rows = [l.split("\t") for l in paf_text.splitlines()]
    assert written == sum(1 for p in paf_rows if p[0] not in lost) and written + skipped == paf_written + paf_skipped
    if not with_targets:
        assert written == paf_written
    rtext = rt.tobytes().decode()
    t0 = {"ref": 0} if not with_targets else dict(zip(T.names, (int(x) for x in T.starts)))
    seen = set()
    for f in mapped:
        s, flag, pos = int(f[0][4:]), int(f[1]), int(f[3])
        read = seq[starts[s]:ends_at[s]].decode()
        rq = qual[starts[s]:ends_at[s]].tobytes().decode()
        orient, oq = (revcomp(read.encode()).decode(), rq[::-1]) if flag & 16 else (read, rq)
        cigar = [(int(n), o) for n, o in re.findall(r"(\d+)([SID=X])", f[5])]
        assert "".join("%d%s" % c for c in cigar) == f[5] and f[6:9] == ["*", "0", "0"]
        tags = dict((t[:2], t[5:]) for t in f[11:])
        assert [t[:4] for t in f[11:]] == ["NM:i", "tp:A", "cm:i", "s1:i"] + (["s2:i"] if not flag & 256 else []) + ["MD:Z", "cs:Z"]
        assert (tags["tp"] == "S") == bool(flag & 256)
        if flag & 256:
            assert (f[9], f[10]) == ("*", "*")
        else:
            assert (f[9], f[10]) == (orient, oq)
            assert sum(n for n, o in cigar if o in "SI=X") == len(f[9])
        assert sum(n for n, o in cigar if o in "SI=X") == len(orient)
        rs = t0[f[2]] + pos - 1
        re_ = rs + sum(n for n, o in cigar if o in "D=X")
        assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", tags["MD"])
        assert ref_from_md(orient, cigar, tags["MD"]) == rtext[rs:re_]
        assert ref_from_cs(orient, cigar, tags["cs"]) == rtext[rs:re_]
        md_edits = sum(len(d) if d else 1 for d, x in re.findall(r"\^([A-Z]+)|([A-Z])", tags["MD"]))
        assert int(tags["NM"]) == md_edits + sum(n for n, o in cigar if o == "I")
        seen |= {o for n, o in cigar} | ({"rev"} if flag & 16 else set()) | ({"sec"} if flag & 256 else set())
    assert {"X", "I", "D", "S", "rev", "sec"} <= seen, seen
    assert unmapped and all(f[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] for f in unmapped)
    for f in unmapped:
        s = int(f[0][4:])
        assert f[9] == seq[starts[s]:ends_at[s]].decode() and f[10] == qual[starts[s]:ends_at[s]].tobytes().decode() and len(f) == 11
