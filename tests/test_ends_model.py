"""CPU: the model of kh_chain_ends (tests/ends_model.py) against the textbook Levenshtein DP of tests/edits_model.py.  For random pairs
with substitutions, indels and Ns: the score of the point the model stops at is the best i - clip_cost * D[i][j] over all cells within
max_edits, the edits it reports are the distance of the two prefixes it aligns, its row turns one prefix into the other with exactly
that many non-'=' bases, and aligned plus clipped bases are the whole end.  Then the hand cases of the definition: the tie that clips,
the cheaper clip cost that extends, a reference that ends first, an insertion as the last base, max_edits = 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cigar_model as CM      # noqa: E402
import ends_model as EM       # noqa: E402
from edits_model import _match  # noqa: E402

C = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def codes(s):
    return [C[c] for c in s]


def dp_table(A, B):
    D = [[0] * (len(B) + 1) for _ in range(len(A) + 1)]
    for j in range(len(B) + 1):
        D[0][j] = j
    for i in range(1, len(A) + 1):
        D[i][0] = i
        for j in range(1, len(B) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (0 if _match(A[i - 1], B[j - 1]) else 1))
    return D


def random_pairs(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = int(rng.integers(0, 41))
        A = [int(x) for x in rng.integers(0, 4, n)]
        B = list(A) + [int(x) for x in rng.integers(0, 4, 40)]
        for _ in range(int(rng.integers(0, 7))):                 # edits anywhere in B's front part
            p = int(rng.integers(0, max(1, n + 2)))
            kind = int(rng.integers(0, 4))
            if kind == 0 and p < len(B):
                B[p] = (B[p] + 1 + int(rng.integers(0, 3))) % 4
            elif kind == 1:
                B.insert(p, int(rng.integers(0, 4)))
            elif kind == 2 and p < len(B):
                del B[p]
            elif p < len(B):
                B[p] = 4
        if n and rng.random() < 0.2:
            A[int(rng.integers(0, n))] = 4
        max_edits = int(rng.choice([0, 1, 2, 5, 31]))
        left = int(rng.choice([0, n // 2, n, n + 40]))            # what the reference has left
        yield A, B[:min(n + max_edits, left)], max_edits, int(rng.choice([1, 2, 3, 4, 7, 255]))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_pairs_against_the_full_matrix(seed):
    for A, B, max_edits, cost in random_pairs(120, seed):
        n = len(A)
        q, r, e, clip, S, runs = EM.extend(A, B, max_edits, cost)
        D = dp_table(A, B)
        best = max(i - cost * D[i][j] for i in range(n + 1) for j in range(len(B) + 1) if D[i][j] <= max_edits)
        assert S == best == q - cost * e, (A, B, max_edits, cost)                         # (i)
        assert D[q][r] == e <= max_edits                                                  # (ii)
        got = CM.apply_ops(A[:q], B[:r], runs)                                            # (iii)
        assert got is not None and got[:2] == (q, r) and got[2] + got[3] + got[4] == e, (A, B, runs)
        assert all(runs[t][0] != runs[t + 1][0] for t in range(len(runs) - 1)) and len(runs) <= 2 * e + 1
        assert q + clip == n and clip >= 0 and 0 <= r <= len(B)                           # (iv)


def ext(a, b, max_edits=31, cost=4, left=None):
    A, B = codes(a), codes(b)
    B = B[:min(len(A) + max_edits, len(B) if left is None else left)]
    q, r, e, clip, S, runs = EM.extend(A, B, max_edits, cost)
    return q, r, e, clip, CM.text(runs)


def test_hand_cases():
    assert EM.end_model(*[np.zeros(0, dtype=np.uint8)] * 2, 0, [5], [5], [0], [0], [0], [5], [9], 4, 31, 4, 0) == (0, 0, 0, 0, [])      # n == 0 rows
    # a mismatch 3 bases from the end: extending gains 3 bases for one edit -- with clip_cost 4 a tie at S = 8, which goes to e = 0
    a, b = "ACGTACGTCATG", "ACGTACGTGATGTTTT"
    assert ext(a, b, cost=4) == (8, 8, 0, 4, "8=")
    assert ext(a, b, cost=3) == (12, 12, 1, 0, "8=1X3=")
    assert ext(a, b, cost=5) == (8, 8, 0, 4, "8=")
    # the reference ends before the read does: the rest is clipped (an insertion costs what it gains at best)
    assert ext("ACGTACGT", "ACGTAC") == (6, 6, 0, 2, "6=")
    assert ext("ACGTACGT", "ACGTACGTAA", left=0) == (0, 0, 0, 8, "")
    # an insertion as the very last base of the read: it cannot pay for itself
    assert ext("ACGTACGTG", "ACGTACGT", cost=1) == (8, 8, 0, 1, "8=")
    # ... but one before the last four bases does
    assert ext("ACGTGACGTA", "ACGTACGTACC", cost=4) == (10, 9, 1, 0, "4=1I5=")
    assert ext("ACGTACGTA", "ACGTGACGTACC", cost=4) == (9, 10, 1, 0, "4=1D5=")
    # max_edits = 0: the exact-match extension and nothing else
    assert ext("ACGTACGTCATG", "ACGTACGTGATG", max_edits=0, cost=1) == (8, 8, 0, 4, "8=")
    assert ext("ACGT", "ACGT", max_edits=0) == (4, 4, 0, 0, "4=")
    # N matches nothing, another N included
    assert ext("ACNTACGTAC", "ACNTACGTACGG", cost=2) == (10, 10, 1, 0, "2=1X7=")
    assert ext("NCGT", "NCGT", cost=4) == (0, 0, 0, 4, "")


def test_rows_strings_and_the_head_in_read_order():
    """the four readers on a text whose both strands are written out by hand; the head's row comes back to front"""
    k = 4
    ref = b"TTGACCAGGTACGTAACCGGTTAGC"
    #                 ^ seed ACGT at 10
    # forward read: 4 bases before the seed with a substitution in the third from it, 7 behind it with a deletion after the third
    read = b"ATGT" + b"ACGT" + b"AACGGTT"                       # the reference has AGGT before the seed and AACCGGTT behind it
    qc, rc = CM._codes(read), CM._codes(ref)
    args = (qc, rc, 0, [4], [10], [0], [0], [0], [0], [len(read)], k, 31, 1)
    assert EM.end_strings(*args[:-1], 0) == (codes("TGTA"), codes("TGGACCAGTT"))           # both read downwards from the seed
    q, r, e, clip, runs = EM.end_model(*args, 0)
    assert (q, r, e, clip, CM.text(runs)) == (4, 4, 1, 0, "1=1X2=")                        # found as 2=1X1=, stored in read order
    q, r, e, clip, runs = EM.end_model(*args, 1)
    assert (q, r, e, clip, CM.text(runs)) == (7, 8, 1, 0, "3=1D4=")                        # AAC-GGTT against AACCGGTT
    # the same read on the other strand: its reverse complement against the same reference, anchored on the same (palindromic) seed
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    rread = read.translate(comp)[::-1]
    assert rread == b"AACCGTT" + b"ACGT" + b"ACAT"
    qc = CM._codes(rread)
    args = (qc, rc, 0, [7], [10], [1], [0], [0], [0], [len(rread)], k, 31, 1)
    assert EM.end_strings(*args[:-1], 0) == (codes("TTGCCAA"), codes("TTGGCCAATCG"))       # A downwards, B the complement upwards
    assert EM.end_strings(*args[:-1], 1) == (codes("ACAT"), codes("ACCTGGTCAA"))           # A upwards, B the complement downwards
    q, r, e, clip, runs = EM.end_model(*args, 0)                # the head of the reversed read is the old tail
    assert (q, r, e, clip, CM.text(runs)) == (7, 8, 1, 0, "4=1D3=")
    q, r, e, clip, runs = EM.end_model(*args, 1)
    assert (q, r, e, clip, CM.text(runs)) == (4, 4, 1, 0, "2=1X1=")
