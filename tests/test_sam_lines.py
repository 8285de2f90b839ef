"""CPU: sam_lines and sam_header over a hand-made Mapping -- the host half of write_sam needs no device: the flags 0, 16, 256, 272 and
2048, POS with targets and with ref_start, '*' for a secondary's SEQ, an unmapped read at its place, a read whose best row is invalid
written as unmapped with its secondary counted as skipped, kept_only=False, unmapped=False, header=False; paf_lines(cs=None) prints
the lines of before and with cs the same lines plus the tag."""
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import orient_model as OM  # noqa: E402

Table = namedtuple("Table", "seg rev q_start q_end r_start r_end count score anchors chain")
READS = [b"ACGTACGTAA", b"GGGGCCCCAT", b"TTTTT", b"ACACACAC", b"CATCATCAT"]
SEQ = b"\n".join(READS) + b"\n"
STARTS = np.cumsum([0] + [len(r) + 1 for r in READS[:-1]])
ENDS = STARTS + np.array([len(r) for r in READS])
QUAL = bytes(33 + i % 40 for i in range(len(SEQ)))
NAMES = ["r%d" % i for i in range(len(READS))]
#        row:   0     1     2     3     4     5     6     7
SEG = [0, 0, 1, 1, 1, 3, 3, 4]                       # read 2 has no row
REV = [0, 1, 1, 0, 1, 0, 0, 0]
FLAG = [3, 2, 3, 2, 3, 3, 2, 0]                      # bit 0 primary, bit 1 kept: row 1 a kept secondary, row 4 a second primary, row 7 not kept
VALID = [1, 1, 1, 1, 1, 0, 1, 1]                     # row 5, the best of read 3, has no whole alignment
BEST = [0, 2, -1, 5, -1]                             # read 4's only row is not kept: no best
RS = [100, 300, 205, 40, 1210, 0, 77, 500]
CIGARS = ["10=", "2S8=", "4=1X5=", "10=", "3=1I6=", "", "8=", "9="]


def mapping():
    u32 = lambda x: np.array(x, dtype=np.uint32)      # noqa: E731
    n = len(SEG)
    table = Table(u32(SEG), np.array(REV, dtype=np.uint8), None, None, None, None, u32(range(3, 3 + n)), np.arange(50, 50 + n, dtype=np.int32), None, None)
    sel = kh.ChainSelect(None, None, np.arange(60, 60 - n, -1, dtype=np.uint8), np.array(FLAG, dtype=np.uint8), np.arange(10, 10 + n, dtype=np.int32), None,
                         np.array(BEST, dtype=np.int32))
    rec = kh.ChainRecords(np.array(VALID, dtype=np.uint8), u32([0] * n), u32([9] * n), u32(RS), u32([r + 10 for r in RS]), u32([10] * n), u32([8] * n), u32([10] * n),
                          u32(range(n)), None, None)
    return kh.Mapping(table, None, None, None, sel, rec)


def csr(rows):
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    return offs, np.frombuffer("".join(rows).encode(), dtype=np.uint8)


def texts():
    """what write_sam hands to sam_lines: every table row's oriented read, then every read as given (a model stands in for the device)"""
    lo = [STARTS[s] for s in SEG] + list(STARTS)
    hi = [ENDS[s] for s in SEG] + list(ENDS)
    rev = REV + [0] * len(READS)
    so, st = OM.oriented_rows(SEQ, lo, hi, rev, True)
    qo, qt = OM.oriented_rows(QUAL, lo, hi, rev, False)
    return (np.array(so, dtype=np.uint64), np.frombuffer(st, dtype=np.uint8)), (np.array(qo, dtype=np.uint64), np.frombuffer(qt, dtype=np.uint8))


def diffs(tag):
    offs, text = csr([tag + str(c) if VALID[c] else "" for c in range(len(SEG))])
    return kh.RecordDiffs(np.array(VALID, dtype=np.uint8), offs, text)


def lines(**kw):
    toff, text = csr(CIGARS)
    seq_rows, qual_rows = texts()
    args = dict(qual_rows=qual_rows, md=diffs("M"), cs=diffs("c"), ref_name="chr", ref_len=5000)
    args.update(kw)
    return kh.sam_lines(mapping(), toff, text, seq_rows, NAMES, **args)


def revcomp(b):
    return b.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_header():
    h = kh.sam_header(ref_name="chr", ref_len=5000).splitlines()
    assert h[0] == "@HD\tVN:1.6\tSO:unsorted" and h[1] == "@SQ\tSN:chr\tLN:5000" and len(h) == 3
    assert h[2].startswith("@PG\tID:kmerhash_amd\tPN:kmerhash_amd\tVN:") and len(h[2].split("\t")) == 4 and h[2].split("VN:")[1]
    T = kh.Targets(["a", "b"], [1000, 2000])
    assert kh.sam_header(T).splitlines()[1:3] == ["@SQ\tSN:a\tLN:1000", "@SQ\tSN:b\tLN:2000"]
    with pytest.raises(ValueError):
        kh.sam_header()
    with pytest.raises(ValueError):
        kh.sam_header(T, ref_name="chr")


def test_lines_flags_and_places():
    out, skipped, n_unmapped = lines()
    assert out[:3] == kh.sam_header(ref_name="chr", ref_len=5000).splitlines()
    f = [l.split("\t") for l in out[3:]]
    assert [(x[0], int(x[1])) for x in f] == [("r0", 0), ("r0", 272), ("r1", 16), ("r1", 256), ("r1", 2048 | 16), ("r2", 4), ("r3", 4), ("r4", 4)]
    assert (skipped, n_unmapped) == (2, 3)              # row 5 (invalid) and row 6, the kept secondary of the read it stands for; row 7 is not kept
    r0, r0s, r1, r1s, r1p = f[:5]
    assert r0[2:9] == ["chr", "101", "60", "10=", "*", "0", "0"] and r0[9] == READS[0].decode() and r0[10] == QUAL[:10].decode()
    assert r0[11:] == ["NM:i:0", "tp:A:P", "cm:i:3", "s1:i:50", "s2:i:10", "MD:Z:M0", "cs:Z:c0"]
    assert r0s[3:6] == ["301", "59", "2S8="] and r0s[9:11] == ["*", "*"] and r0s[11:] == ["NM:i:1", "tp:A:S", "cm:i:4", "s1:i:51", "MD:Z:M1", "cs:Z:c1"]
    assert r1[9] == revcomp(READS[1]).decode() and r1[10] == QUAL[STARTS[1]:ENDS[1]][::-1].decode() and r1[3] == "206"
    assert r1s[9:11] == ["*", "*"] and r1p[9] == revcomp(READS[1]).decode() and r1p[3] == "1211" and "s2:i:14" in r1p
    assert f[5] == ["r2", "4", "*", "0", "0", "*", "*", "0", "0", READS[2].decode(), QUAL[STARTS[2]:ENDS[2]].decode()]
    assert f[6][9] == READS[3].decode() and f[7][9] == READS[4].decode()


def test_options():
    base, _, _ = lines()
    out, skipped, n_unmapped = lines(header=False)
    assert out == base[3:]
    out, skipped, n_unmapped = lines(unmapped=False, header=False)
    assert [l.split("\t")[0] for l in out] == ["r0", "r0", "r1", "r1", "r1"] and (skipped, n_unmapped) == (2, 3)
    out, skipped, n_unmapped = lines(kept_only=False, header=False)
    assert [(l.split("\t")[0], int(l.split("\t")[1])) for l in out][-1] == ("r4", 4) and (skipped, n_unmapped) == (3, 3)      # row 7 is looked at now; read 4 still has no best
    out, _, _ = lines(qual_rows=None, md=None, cs=None, header=False)
    assert out[0].split("\t")[10] == "*" and out[0].split("\t")[-1] == "s2:i:10" and out[5].split("\t")[10] == "*"
    out, _, _ = lines(ref_start=100, header=False)
    assert [l.split("\t")[3] for l in out[:5]] == ["1", "201", "106", "-59", "1111"]


def test_targets_name_the_row_and_make_pos_local():
    T = kh.Targets(["a", "b"], [1000, 2000], spacer=64)      # b covers [1064, 3064)
    out, skipped, n_unmapped = lines(ref_name=None, ref_len=None, targets=T, header=False)
    f = [l.split("\t") for l in out]
    assert [(x[0], x[2], x[3]) for x in f[:5]] == [("r0", "a", "101"), ("r0", "a", "301"), ("r1", "a", "206"), ("r1", "a", "41"), ("r1", "b", "147")]
    with pytest.raises(ValueError):
        lines(targets=T)
    with pytest.raises(ValueError):
        lines(ref_name=None, ref_len=None, targets=T, ref_start=5)


def test_a_row_that_does_not_walk_the_texts_is_an_error():
    bad = diffs("M")
    bad.ok[0] = 0
    with pytest.raises(ValueError, match="ref_order=True"):
        lines(md=bad)


def test_paf_lines_with_and_without_cs():
    toff, text = csr(CIGARS)
    before, skipped = kh.paf_lines(mapping(), toff, text, NAMES, "chr", 5000)
    same, _ = kh.paf_lines(mapping(), toff, text, NAMES, "chr", 5000, cs=None)
    assert same == before and skipped == 1 and len(before) == 6 and all(l.split("\t")[-1].startswith("cg:Z:") for l in before)
    tagged, skipped = kh.paf_lines(mapping(), toff, text, NAMES, "chr", 5000, cs=diffs("c"))
    kept = [c for c in range(len(SEG)) if FLAG[c] & 2 and VALID[c]]
    assert tagged == [l + "\tcs:Z:c%d" % c for l, c in zip(before, kept)] and skipped == 1
