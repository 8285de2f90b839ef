"""CPU: the model of kh_chain_cigars (tests/cigar_model.py) against the textbook Levenshtein DP of tests/edits_model.py.  The canonical
recurrence -- candidates dropped, not clamped, ties to X, then I, then D -- must find the distance, and its traceback must be a valid
alignment: the ops applied to A give B under the match rule, X + I + D is the distance, a row has at most 2 d + 1 runs and no two equal
neighbours.  Random pairs up to 70 bases with N, lower case and two-letter strings, the hand cases of the definition, and an edit at the
first and at the last base."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cigar_model as CM  # noqa: E402
import edits_model as EM  # noqa: E402


def codes(s):
    return [EM.code(b) for b in s]


def check_pair(a, b):
    A, B = codes(a), codes(b)
    d = EM.lev(A, B)
    got = CM.canonical(A, B, CM.DMAX)
    if d > CM.DMAX or abs(len(A) - len(B)) > CM.DMAX:
        assert got is None, (a, b, d)
        return None
    assert got is not None, (a, b, d)
    e, runs = got
    assert e == d, (a, b, d, e, CM.text(runs))
    walked = CM.apply_ops(A, B, runs)
    assert walked is not None, (a, b, CM.text(runs))
    i, j, x, ins, dels = walked
    assert (i, j) == (len(A), len(B)) and x + ins + dels == d, (a, b, CM.text(runs))
    assert len(runs) <= 2 * d + 1 and all(p[0] != q[0] for p, q in zip(runs, runs[1:])), (a, b, CM.text(runs))
    # the distance is found at the first level that reaches the target: a smaller bound finds nothing, the exact one the same row
    assert CM.canonical(A, B, d) == got
    assert d == 0 or CM.canonical(A, B, d - 1) is None
    return CM.text(runs)


def mutate(rng, a, rate, alphabet):
    b = bytearray()
    for c in a:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            b.append(rng.choice(alphabet))
        b.append(rng.choice(alphabet) if 2 * rate / 3 <= u < rate else c)
    return bytes(b)


@pytest.mark.parametrize("alphabet", [b"ACGT", b"AC", b"ACGTN", b"ACGTacgt"])
def test_random_pairs_against_the_textbook_dp(alphabet):
    rng = random.Random(len(alphabet))
    seen = set()
    for t in range(400):
        a = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 71)))
        if t % 4 == 0:
            b = bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 71)))          # unrelated: often beyond 31
        else:
            b = mutate(rng, a, rng.choice([0.0, 0.03, 0.1, 0.2, 0.4]), alphabet)
        s = check_pair(a, b)
        seen.add("over" if s is None else "exact" if set(s) <= set("0123456789=") else "edits")
    assert seen == {"over", "exact", "edits"}


def test_hand_cases():
    assert check_pair(b"ACGTAC", b"ACTAC") == "2=1I3="
    assert check_pair(b"AAA", b"AA") == "2=1I"
    assert check_pair(b"AC", b"CA") == "2X"
    assert check_pair(b"", b"") == "" and check_pair(b"ACGT", b"ACGT") == "4=" and check_pair(b"", b"AC") == "2D" and check_pair(b"AC", b"") == "2I"
    assert check_pair(b"N", b"N") == "1X" and check_pair(b"acgt", b"ACGT") == "4="


def test_an_edit_at_the_first_and_at_the_last_base():
    a = b"ACGTTGCATGCAAGCT"
    assert check_pair(a, b"T" + a[1:]) == "1X15="
    assert check_pair(a, a[:-1] + b"A") == "15=1X"
    assert check_pair(a, a[1:]) == "1I15="
    assert check_pair(a, a[:-1]) == "15=1I"
    assert check_pair(a, b"G" + a) == "1D16="
    assert check_pair(a, a + b"G") == "16=1D"


def test_reverse_strand_rows_read_the_complement():
    # B lies in rtext as the reverse complement of what A faces; the model orients it before it aligns
    a, b = b"ACGTAC", b"GTAGT"                                     # revcomp(b) = ACTAC
    assert CM.canonical(codes(a), EM._oriented(codes(b), 1), 31) == (1, CM.parse("2=1I3="))


def test_parse_and_text_round_trip():
    for s in ("", "5=", "2=1I3=", "1X15=", "3D2I7="):
        assert CM.text(CM.parse(s)) == s
    with pytest.raises(AssertionError):
        CM.parse("3M")
