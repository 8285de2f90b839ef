"""CPU: the model of kh_mate_rescue (tests/rescue_model.py) against the hand-written cases of tests/rescue_cases.py and against brute
force on small random inputs over ACGTN: d* is the least Levenshtein distance of R to any substring of the window, e and last are the
extremes of the end columns attaining it, and the row consumes m and re - rs bases, replays R into the reference stretch and holds d*
edit bases."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rescue_model as RM  # noqa: E402
from cigar_model import OP_D, OP_I, OP_X, _codes, apply_ops, parse  # noqa: E402
from edits_model import _match  # noqa: E402
from rescue_cases import CASES  # noqa: E402


def runs_of(offsets, ops, j):
    return [(int(v) & 15, int(v) >> 4) for v in ops[int(offsets[j]):int(offsets[j + 1])]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_written_cases(case):
    _, qt, rt, base, me, (q_lo, q_hi, w_lo, w_hi, rev), (edits, rs, re, span, cigar) = case
    got = RM.rescue_model(qt, rt, [q_lo], [q_hi], [w_lo], [w_hi], [rev], base, me)
    assert (int(got[0][0]), int(got[1][0]), int(got[2][0]), int(got[3][0])) == (edits, rs, re, span)
    assert runs_of(got[4], got[5], 0) == parse(cigar)


def lev(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (0 if _match(a[i - 1], b[j - 1]) else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def test_against_brute_force():
    rng = random.Random(26)
    seen = set()
    for it in range(160):
        m, W = rng.randrange(1, 13), rng.randrange(0, 31)
        alpha = b"ACGTN" if it % 3 else b"AC"
        win = bytes(rng.choice(alpha) for _ in range(W))
        if W >= m and it % 2:                       # a planted copy with a few edits
            s = rng.randrange(0, W - m + 1)
            mate = bytearray(win[s:s + m])
            for _ in range(rng.randrange(0, 4)):
                mate[rng.randrange(m)] = rng.choice(alpha)
            mate = bytes(mate)
        else:
            mate = bytes(rng.choice(alpha) for _ in range(m))
        rev, base, pad = it & 1, rng.choice([0, 7]), rng.randrange(0, 4)
        qt = b"T" * pad + (bytes(reversed(mate.translate(bytes.maketrans(b"ACGT", b"TGCA")))) if rev else mate) + b"G"
        rt = b"C" * pad + win + b"A"
        me = rng.choice([31, 31, 3, 0])
        edits, rs, re, span, offsets, ops = RM.rescue_model(qt, rt, [pad], [pad + m], [base + pad], [base + pad + W], [rev], base, me)
        R, wc = [int(x) for x in _codes(mate)], [int(x) for x in _codes(win)]
        assert RM.pattern(_codes(qt), pad, pad + m, rev) == R
        by_end = [min(lev(R, wc[a:b]) for a in range(b + 1)) for b in range(W + 1)]
        d = min(by_end)
        if d > me:
            assert (int(edits[0]), int(rs[0]), int(re[0]), int(span[0]), len(ops)) == (RM.OVER, 0, 0, 0, 0)
            seen.add("over")
            continue
        cols = [b for b, v in enumerate(by_end) if v == d]
        e, s = int(re[0]) - base - pad, int(rs[0]) - base - pad
        assert int(edits[0]) == d and e == cols[0] and int(span[0]) == cols[-1] - cols[0]
        runs = runs_of(offsets, ops, 0)
        assert 0 <= s <= e and len(runs) <= 2 * d + 1 and all(a[0] != b[0] for a, b in zip(runs, runs[1:]))
        walked = apply_ops(R, wc[s:e], runs) if runs else (0, 0, 0, 0, 0)
        assert walked is not None and walked[0] == m and walked[1] == e - s and walked[2] + walked[3] + walked[4] == d
        assert sum(n for op, n in runs if op in (OP_X, OP_I, OP_D)) == d
        seen.add("d%d" % min(d, 2))
        if span[0] > 0:
            seen.add("tie")
    assert {"over", "d0", "d1", "d2", "tie"} <= seen


def test_a_request_that_is_not_looked_at_and_the_shape_of_a_whole_call():
    qt, rt = b"ACGTACGTAC", b"TTACGTACGTACTT"
    got = RM.rescue_model(qt, rt, [0, 0, 4, 0], [10, 11, 4, 10], [0, 0, 0, 3], [14, 14, 14, 2], [0, 0, 0, 0])
    assert got[0].tolist() == [0, RM.NONE, RM.NONE, RM.NONE] and got[0].dtype == np.int32
    assert got[1].tolist() == [2, 0, 0, 0] and got[2].tolist() == [12, 0, 0, 0] and got[4].tolist() == [0, 1, 1, 1, 1]
    assert [x.dtype for x in got[1:]] == [np.uint32, np.uint32, np.uint32, np.uint64, np.uint32]
    # 513 bases are one too many; 512 are looked at
    long = b"A" * 513
    assert RM.rescue_model(long, long, [0, 0], [513, 512], [0, 0], [513, 513], [0, 0])[0].tolist() == [RM.NONE, 0]
