"""CPU: the model of kh_fastq_records and kh_pack_rows (tests/fastq_model.py) against an independent statement.  For the well-formed
cases of tests/fastq_cases.py the columns must be the slices raw.split(b"\\n") gives, and the seq of read_fastq per the model must be
b"\\n".join(seqs) + b"\\n"; the malformed cases are held to their status words, with every record after a bad one numbered and
intact; the pack model is held to numpy slicing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fastq_cases as FC  # noqa: E402
import fastq_model as FM  # noqa: E402

WELL_FORMED = sorted(n for n, c in FC.CASES.items() if all(r[0][:1] == b"@" and r[2][:1] == b"+" and len(r[1]) == len(r[3]) and r[0][1:].split() and
                                                            r[0][1:2] not in (b" ", b"\t") for r in c.recs) and not n.startswith("tail") and (c.recs or n in ("empty", "one_newline")))


def name_of(header, strip):
    name = header[1:].replace(b"\t", b" ").split(b" ")[0]
    return name[:-2] if strip and len(name) > 2 and name[-2:] in (b"/1", b"/2") else name


@pytest.mark.parametrize("strip", [False, True], ids=["as_written", "strip_mate"])
@pytest.mark.parametrize("case", WELL_FORMED)
def test_well_formed_cases_are_the_split_lines(case, strip):
    c = FC.CASES[case]
    raw = c.text
    rows, n_bad, tail = FM.fastq_records(raw, FM.STRIP_MATE if strip else 0)
    lines = [l[:-1] if l.endswith(b"\r") else l for l in raw.split(b"\n")]
    assert (len(rows), n_bad, tail) == (len(c.recs), 0, 0)
    for r, (name_lo, name_hi, s0, s1, q0, st) in enumerate(rows):
        assert st == 0
        assert (raw[s0:s1], raw[q0:q0 + s1 - s0]) == (lines[4 * r + 1], lines[4 * r + 3]) == (c.recs[r][1], c.recs[r][3])
        assert raw[name_lo:name_hi] == name_of(lines[4 * r], strip)
        assert raw[name_lo - 1:name_lo] == b"@" and (s0 == 0 or raw[s0 - 1:s0] == b"\n") and raw[q0 - 1:q0] == b"\n"
    got = FM.read_fastq([raw], strip)
    assert got["seq"] == b"".join(r[1] + b"\n" for r in c.recs) == (b"\n".join(r[1] for r in c.recs) + b"\n" if c.recs else b"")
    assert got["qual"] == b"".join(r[3] + b"\n" for r in c.recs)
    assert [got["seq"][a:b] for a, b in zip(got["read_starts"], got["read_ends"])] == [r[1] for r in c.recs]
    assert got["read_starts"][:1] in ([], [0]) and all(a == b + 1 for a, b in zip(got["read_starts"][1:], got["read_ends"]))
    off, text = got["names"]
    assert [text[a:b] for a, b in zip(off, off[1:])] == [name_of(r[0], strip) for r in c.recs]


def test_the_cases_cover_what_they_are_there_for():
    assert len(WELL_FORMED) >= 15 and {"crlf", "many", "straddle", "names", "blank_trailing_line", "empty_sequence", "quality_of_acgt"} <= set(WELL_FORMED)
    stripped = [bytes(FC.CASES["names"].text[a:b]) for a, b, *_ in FM.fastq_records(FC.CASES["names"].text, 1)[0]]
    assert stripped == [b"with", b"tab", b"x", b"frag7", b"frag7", b"/1", b"a/3", b"/2"]
    assert len(FC.CASES["many"].text) > 20 * FC.TILE and len(FC.CASES["straddle"].text) > 5 * FC.TILE


EXPECT = {      # case -> (status per record, tail lines)
    "tail1": ([0, 0, 0], 1), "tail2": ([0, 0, 0], 2), "tail3": ([0, 0, 0], 3), "blank_trailing_crlf": ([0, 0, 0], 0),
    "empty_name": ([0, 8, 8, 0], 0), "missing_at": ([0, 1, 0], 0), "missing_plus": ([0, 2, 2, 0], 0), "length_mismatch": ([0, 4, 4, 0], 0),
    "empty_header_line": ([0, 9, 0], 0), "only_newlines": ([11, 11], 0), "one_newline": ([], 0), "no_newline_at_all": ([], 1), "empty": ([], 0),
}


@pytest.mark.parametrize("case", sorted(EXPECT))
def test_malformed_cases_keep_their_records_numbered(case):
    c = FC.CASES[case]
    rows, n_bad, tail = FM.fastq_records(c.text)
    status, want_tail = EXPECT[case]
    assert ([r[5] for r in rows], tail, n_bad) == (status, want_tail, sum(1 for s in status if s))
    for r, (name_lo, name_hi, s0, s1, q0, st) in enumerate(rows):
        if st:
            assert s1 == s0 and q0 == s0      # kept, as an empty read
        elif c.recs:
            assert (c.text[s0:s1], c.text[q0:q0 + s1 - s0], c.text[name_lo:name_hi]) == (c.recs[r][1], c.recs[r][3], name_of(c.recs[r][0], False))
    got = FM.read_fastq([c.text])
    assert got["n_reads"] == len(status) and [b - a for a, b in zip(got["read_starts"], got["read_ends"])] == [0 if s else len(r[1]) for s, r in zip(status, c.recs or [None] * 9)]


def test_two_texts_interleave_and_share_names():
    one, two, r1, r2 = FC.pair_texts()
    got = FM.read_fastq([one, two])
    want = [r[1] for pair in zip(r1, r2) for r in pair]
    assert [got["seq"][a:b] for a, b in zip(got["read_starts"], got["read_ends"])] == want and got["seq"] == b"".join(s + b"\n" for s in want)
    off, text = got["names"]
    assert [text[a:b] for a, b in zip(off, off[1:])] == [b"frag%d" % (s // 2) for s in range(len(want))]
    short = FM.read_fastq([one, FC.write(r2[:-3])])      # the shorter text is filled up with empty reads
    assert short["n_reads"] == len(want) and short["counts"] == [len(r1), len(r2) - 3]
    assert [b - a for a, b in zip(short["read_starts"], short["read_ends"])][-6:] == [len(r1[-3][1]), 0, len(r1[-2][1]), 0, len(r1[-1][1]), 0]


def test_pack_model_against_slicing():
    text, lo, hi, dst, out_len = FC.pack_case()
    assert sorted(set(int(h - l) for l, h in zip(lo, hi))) == sorted(FC.ROW_LENGTHS)
    assert {(int(l) % 8, int(d) % 8) for l, d in zip(lo, dst)} == {(a, b) for a in range(8) for b in range(8)}
    for sep in (-1, 0, 10, 255):
        out = np.frombuffer(FM.pack_rows(bytes(text), lo.tolist(), hi.tolist(), dst.tolist(), sep, bytearray(b"\xfe" * out_len)), dtype=np.uint8)
        want = np.full(out_len, 0xfe, dtype=np.uint8)
        for l, h, d in zip(lo.tolist(), hi.tolist(), dst.tolist()):
            want[d:d + h - l] = text[l:h]
            if sep >= 0:
                want[d + h - l] = sep
        assert np.array_equal(out, want) and (want == 0xfe).sum() > 100
    # rows out of the text are empty rows (their separator is still written); stores stop at the end of out
    out = FM.pack_rows(b"abcdefgh", [2, 6, 5, 0], [5, 9, 4, 8], [0, 4, 6, 8], 10, bytearray(b"\xfe" * 12))
    assert bytes(out) == b"cde\n\n\xfe\n\xfeabcd"
