"""CPU: tests/diffs_model.py and tests/orient_model.py, the yardsticks of kh_record_diffs and kh_oriented_rows, against hand-written rows
with their cs and MD written out, and against an independent check on planted alignments: from the oriented read, the row and its MD --
and, separately, from its cs alone -- the reference bases the row covers are rebuilt and compared with the text.  The model is what the
GPU tests compare the kernels with; this test needs neither a GPU nor the library."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import diffs_cases as DC  # noqa: E402
import diffs_model as DM  # noqa: E402
import orient_model as OM  # noqa: E402
from diffs_cases import D, EQ, I, M, S, X, run  # noqa: E402

MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
#        0123456789
READ = b"ACGTACGTAC"
REF = b"xxACGTTCGTACGG"      # reference coordinates 100.. : ref_base = 100


def one(runs, kind, rev=0, lo=0, hi=10, rs=102, valid=1, read=READ, ref=REF):
    return DM.row_text(read, ref, 100, [run(o, l) for o, l in runs], valid, rev, lo, hi, rs, kind)


@pytest.mark.parametrize("runs,cs,md", [
    ([(EQ, 10)], b":10", b"10"),
    ([(EQ, 4), (X, 1), (EQ, 5)], b":4*ta:5", b"4T5"),
    ([(X, 1), (EQ, 9)], b"*aa:9", b"0A9"),                              # starts with an edit: MD starts with 0 (X need not differ)
    ([(EQ, 9), (X, 1)], b":9*cc", b"9C0"),                              # ends with one
    ([(EQ, 3), (I, 2), (EQ, 5)], b":3+ta:5", b"8"),                     # the matches around an insertion make one number
    ([(EQ, 3), (D, 2), (EQ, 7)], b":3-tt:7", b"3^TT7"),
    ([(EQ, 2), (X, 1), (D, 1), (X, 2), (EQ, 5)], b":2*gg-t*tt*ca:5", b"2G0^T0T0C5"),      # neighbouring edits have 0 between them
    ([(S, 2), (EQ, 6), (S, 2)], b":6", b"6"),
    ([(S, 10)], b"", b"0"),
    ([(EQ, 4), (X, 0), (M, 0), (EQ, 6)], b":4:6", b"10"),              # runs of length 0 vanish; cs keeps the two runs apart
])
def test_hand_rows(runs, cs, md):
    assert one(runs, DM.CS) == cs
    assert one(runs, DM.MD) == md
    assert MD_RE.fullmatch(md.decode())


def test_reverse_rows_complement_the_read_and_keep_what_is_no_base():
    # the read as stored: "aCNT-" -> oriented: complement of '-', T, N, C, a = n, A, N, G, t -> codes 4, 0, 4, 2, 3
    assert DM.oriented(b"aCNT-", 0, 5, 1) == [4, 0, 4, 2, 3]
    assert DM.oriented(b"aCNT-", 0, 5, 0) == [0, 1, 4, 3, 4]
    assert one([(X, 5)], DM.CS, rev=1, hi=5, rs=100, read=b"aCNT-", ref=b"g*Ntc") == b"*gn*na*nn*tg*ct"
    assert one([(X, 2), (D, 3)], DM.MD, rev=1, hi=2, rs=100, read=b"aC", ref=b"g*Ntc") == b"0G0N0^NTC0"


@pytest.mark.parametrize("over", [dict(valid=0), dict(hi=9), dict(hi=11, read=READ + b"A"), dict(rs=99), dict(rs=105), dict(lo=3, hi=2), dict(hi=11)])
def test_rows_that_are_not_good(over):
    for kind in (DM.CS, DM.MD):
        assert one([(EQ, 10)], kind, **over) is None
    assert one([(EQ, 10)], DM.CS, rs=104) == b":10"                  # the last base of the text
    assert one([(EQ, 4), (M, 2), (EQ, 4)], DM.CS) is None and one([(EQ, 4), (3, 2), (EQ, 4)], DM.MD) is None and one([], DM.MD) is None


def rebuild_from_md(o, runs, md):
    m, qi = [], 0
    for v in runs:
        op, l = v & 15, v >> 4
        if op in (S, I):
            qi += l
        elif op in (EQ, X):
            m += list(o[qi:qi + l]); qi += l
        else:
            m += [None] * l
    at = 0
    for num, dele, sub in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            at += int(num)
        elif dele:
            assert m[at:at + len(dele)] == [None] * len(dele)
            m[at:at + len(dele)] = list(dele); at += len(dele)
        else:
            m[at] = sub; at += 1
    assert at == len(m)
    return "".join(m)


def rebuild_from_cs(o, runs, cs):
    qi = (runs[0] >> 4) if runs[0] & 15 == S else 0
    out = []
    for tok in re.findall(r":\d+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+", cs):
        if tok[0] == ":":
            out.append(o[qi:qi + int(tok[1:])]); qi += int(tok[1:])
        elif tok[0] == "*":
            assert o[qi] == tok[2].upper()
            out.append(tok[1].upper()); qi += 1
        elif tok[0] == "+":
            qi += len(tok) - 1
        else:
            out.append(tok[1:].upper())
    return "".join(out)


def test_planted_alignments_give_back_the_reference():
    a, spans = DC.planted(3)
    res = {k: DM.record_diffs(a["qtext"], a["rtext"], a["ref_base"], a["offsets"], a["ops"], a["valid"], a["rev"], a["q_lo"], a["q_hi"], a["rs"], k) for k in (DM.CS, DM.MD)}
    assert all(res[DM.CS]["ok"]) and all(res[DM.MD]["ok"])
    q, rt = a["qtext"].tobytes(), a["rtext"].tobytes().decode()
    seen = set()
    for c, (rs, re_) in enumerate(spans):
        runs = [int(v) for v in a["ops"][int(a["offsets"][c]):int(a["offsets"][c + 1])]]
        o = "".join("ACGTN"[x] for x in DM.oriented(q, int(a["q_lo"][c]), int(a["q_hi"][c]), int(a["rev"][c])))
        row = lambda r: r["text"][r["offsets"][c]:r["offsets"][c + 1]].decode()      # noqa: E731
        md, cs = row(res[DM.MD]), row(res[DM.CS])
        want = rt[rs - a["ref_base"]:re_ - a["ref_base"]]
        assert MD_RE.fullmatch(md)
        assert rebuild_from_md(o, runs, md) == want, c
        assert rebuild_from_cs(o, runs, cs) == want, c
        seen |= {v & 15 for v in runs} | {"rev"} if a["rev"][c] else {v & 15 for v in runs}
    assert {S, EQ, X, I, D, "rev"} <= seen


def test_orient_model():
    text = b"ACGTNacgtn!"
    offs, out = OM.oriented_rows(text, [0, 0, 2, 9, 5], [11, 11, 4, 20, 3], [0, 1, 3, 1, 1], True)
    assert offs == [0, 11, 22, 24, 26, 26]
    assert out == text + b"!nacgtNACGT" + b"AC" + b"!n"
    assert OM.oriented_rows(text, [0], [11], [1], False) == ([0, 11], text[::-1])
