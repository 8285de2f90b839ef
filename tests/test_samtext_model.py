"""CPU: tests/samtext_model.py, the yardstick of kh_sam_lines, against lines written out by hand: a mapped line with every tag, a
secondary ('*' for SEQ and QUAL, no s2), an unmapped line of exactly 11 fields, a paired line with '=' and a negative TLEN; what a row
index outside its CSR prints; and the numbers against "%d"."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import samtext_model as SM  # noqa: E402


def csr(rows):
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + len(r))
    return offs, b"".join(rows)


NAMES, TNAMES = csr([b"read/1", b"r2"]), csr([b"chr1", b"chrM"])
CIGAR, SEQ, QUAL = csr([b"3S7=", b"10="]), csr([b"ACGTACGTAA", b"", b"GGGGCCCCAT"]), csr([b"IIIIIHHHH#", b"", b"#########!"])
MD, CS = csr([b"7", b"4A5"]), csr([b":7", b":4*at:5"])


def one(**c):
    base = dict(name=0, flag=0, rname=0, pos=1, mapq=0, cigar=0, rnext=-1, pnext=0, tlen=0, seq=0, qual=0, tags=0, nm=0, tp=ord("P"), cm=0, s1=0, s2=0, md=0, cs=0)
    base.update(c)
    offs, text = SM.sam_lines(NAMES, TNAMES, CIGAR, SEQ, QUAL, MD, CS, {k: [v] for k, v in base.items()})
    assert offs == [0, len(text)]
    return text


def test_a_mapped_line_with_every_tag():
    got = one(flag=16, pos=101, mapq=60, tags=15, nm=1, cm=12, s1=93, s2=-4)
    assert got == b"read/1\t16\tchr1\t101\t60\t3S7=\t*\t0\t0\tACGTACGTAA\tIIIIIHHHH#\tNM:i:1\ttp:A:P\tcm:i:12\ts1:i:93\ts2:i:-4\tMD:Z:7\tcs:Z::7\n"


def test_a_secondary_has_stars_and_no_s2():
    got = one(name=1, flag=256, rname=1, pos=7, cigar=1, seq=-1, qual=-1, tags=SM.TAG_BASE | SM.TAG_MD | SM.TAG_CS, nm=1, tp=ord("S"), cm=4, s1=51, s2=9, md=1, cs=1)
    assert got == b"r2\t256\tchrM\t7\t0\t10=\t*\t0\t0\t*\t*\tNM:i:1\ttp:A:S\tcm:i:4\ts1:i:51\tMD:Z:4A5\tcs:Z::4*at:5\n"


def test_an_unmapped_line_has_exactly_eleven_fields():
    got = one(name=1, flag=4, rname=-1, pos=0, cigar=-1, seq=2, qual=2, nm=5, s1=7)
    assert got == b"r2\t4\t*\t0\t0\t*\t*\t0\t0\tGGGGCCCCAT\t#########!\n" and got.count(b"\t") == 10 and not got.endswith(b"\t\n")


def test_a_paired_line_with_the_same_target_and_a_negative_tlen():
    got = one(flag=147, pos=5401, mapq=60, cigar=1, rnext=SM.RNEXT_SAME, pnext=5101, tlen=-400, tags=SM.TAG_BASE | SM.TAG_S2, s1=95)
    assert got == b"read/1\t147\tchr1\t5401\t60\t10=\t=\t5101\t-400\tACGTACGTAA\tIIIIIHHHH#\tNM:i:0\ttp:A:P\tcm:i:0\ts1:i:95\ts2:i:0\n"
    assert one(rnext=1).split(b"\t")[6] == b"chrM"


def test_rows_outside_their_csr_and_empty_rows():
    f = one(name=2, rname=2, cigar=-1, rnext=7, seq=3, qual=-5, tags=12, md=2, cs=-1).rstrip(b"\n").split(b"\t")
    assert [f[0], f[2], f[5], f[6], f[9], f[10]] == [b"*"] * 6 and f[11:] == [b"MD:Z:", b"cs:Z:"]
    assert one(seq=1, qual=1).split(b"\t")[9:11] == [b"*", b"*\n"]      # an empty SEQ / QUAL row is '*'
    offs, text = SM.sam_lines(csr([b""]), None, None, None, None, None, None, {k: [0] for k in SM.COLUMNS})
    assert text == b"\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"                    # an empty name prints nothing; absent CSRs print '*'
    offs, text = SM.sam_lines(NAMES, TNAMES, CIGAR, SEQ, None, None, None, {k: [] for k in SM.COLUMNS})
    assert (offs, text) == ([0], b"")


def test_offsets_that_leave_the_text_are_clamped():
    assert SM.row(([0, 3, 99], b"abcdef"), 1) == (True, b"def") and SM.row(([4, 2], b"abcdef"), 0) == (True, b"")


@pytest.mark.parametrize("v", [0, 9, 10, 99, 100, 2 ** 31 - 1, 2 ** 32 - 1, -1, -2 ** 31])
def test_numbers_are_what_percent_d_prints(v):
    assert SM.decimal(v) == ("%d" % v).encode()
    if v >= 0:
        assert one(flag=v, pos=v, pnext=v).split(b"\t")[1::2][:2] == [b"%d" % v] * 2 and one(pnext=v).split(b"\t")[7] == b"%d" % v
    if -2 ** 31 <= v < 2 ** 31:
        assert one(tlen=v, tags=3, s1=v, s2=v).rstrip(b"\n").split(b"\t")[8::6] == [b"%d" % v, b"s1:i:%d" % v]
