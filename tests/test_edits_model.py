"""CPU: the model of kh_chain_edits (tests/edits_model.py) against itself: the banded distance the long GPU cases are compared with
equals the full matrix wherever the distance is within max_edits and says OVER beyond it, on random short pairs with substitutions and
indels, both strands, N and lower case; the hand cases of the definition."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edits_model as EM  # noqa: E402


def codes(s):
    return [EM.code(b) for b in s]


def revcomp(s):
    return bytes({65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97}.get(b, b) for b in reversed(s))


def mutate(rng, s, rate):
    out = bytearray()
    for b in s:
        u = rng.random()
        if u < rate / 3:
            continue                                             # deletion
        if u < 2 * rate / 3:
            out.append(rng.choice(list(b"ACGT")))                # insertion before b
        if u < rate and u >= 2 * rate / 3:
            out.append(rng.choice([c for c in b"ACGTN" if c != b]))   # substitution (sometimes by N)
        else:
            out.append(b)
    return bytes(out)


def test_code_table():
    assert codes(b"ACGTacgt") == [0, 1, 2, 3, 0, 1, 2, 3]
    assert all(EM.code(b) == 4 for b in range(256) if bytes([b]) not in (b"A", b"C", b"G", b"T", b"a", b"c", b"g", b"t"))


def test_hand_cases():
    A = codes(b"ACGTACGT")
    assert EM.lev(A, A) == 0
    assert EM.lev(A, codes(b"ACGAACGT")) == 1                  # substitution
    assert EM.lev(A, codes(b"ACGTTACGT")) == 1                 # insertion
    assert EM.lev(A, codes(b"ACGACGT")) == 1                   # deletion
    assert EM.lev(codes(b"ACNT"), codes(b"ACNT")) == 1         # N matches nothing, another N included
    assert EM.lev(codes(b"acgt"), codes(b"ACGT")) == 0         # case is folded
    assert EM.lev(A, codes(revcomp(b"ACGTACGT")), 1) == 0      # reverse strand: B lies in the text as A's reverse complement
    assert EM.lev(codes(b"AACC"), codes(b"GGTT"), 1) == 0
    assert EM.lev(codes(b"AACC"), codes(b"GNTT"), 1) == 1
    assert EM.lev(codes(b"A"), codes(b"AC")) == 1 and EM.lev(codes(b"AC"), codes(b"A")) == 1
    for me in (0, 1, 5):
        assert EM.lev_banded(A, A, 0, me) == 0
    assert EM.lev_banded(A, codes(b"ACGAACGT"), 0, 0) == EM.OVER
    assert EM.lev_banded(A, codes(b"ACGAACGT"), 0, 1) == 1
    assert EM.lev_banded(A, codes(b"ACG"), 0, 4) == EM.OVER    # |dq - dr| > max_edits


def test_banded_equals_full_matrix():
    rng = np.random.default_rng(5)
    import random
    pr = random.Random(5)
    seen = {"over": 0, "exact": 0, "indel": 0}
    for t in range(3000):
        n = int(rng.integers(1, 41))
        a = bytes(rng.choice(list(b"ACGT"), n).tolist())
        if t % 7 == 0:
            a = a.lower()
        if t % 11 == 0:
            a = a[: n // 2] + b"N" + a[n // 2 + 1:]
        b = mutate(pr, a, [0.0, 0.05, 0.15, 0.4][t % 4]) or b"A"
        rv = t & 1
        B = codes(revcomp(b)) if rv else codes(b)
        full = EM.lev(codes(a), B, rv)
        for me in (0, 1, 3, 8, 31):
            got = EM.lev_banded(codes(a), B, rv, me)
            assert got == (full if full <= me else EM.OVER), (a, b, rv, me, full, got)
            seen["over" if got == EM.OVER else "exact"] += 1
        seen["indel"] += len(a) != len(b)
    assert min(seen.values()) > 300, seen


def test_link_and_call_model():
    q = b"ACGTACGTACGTAAAC"
    r = b"TTACGTACGAACGTAAAC"                                   # q with one substitution, at ref_base 100 - 2
    qpos, rpos = np.array([0, 4, 12], dtype=np.uint32), np.array([100, 104, 112], dtype=np.uint32)
    rev, pred, chain = np.zeros(3, dtype=np.uint8), np.array([-1, 0, 1], dtype=np.int32), np.zeros(3, dtype=np.int32)
    for banded in (False, True):
        link, edits, over = EM.chain_edits_model(q, r, qpos, rpos, rev, pred, chain, 1, 4, ref_base=98, max_edits=2, banded=banded)
        assert link.tolist() == [EM.NOLINK, 0, 1] and edits.tolist() == [1] and over.tolist() == [0]
    link, edits, over = EM.chain_edits_model(q, r, qpos, rpos, rev, pred, chain, 1, 4, ref_base=98, max_edits=0)
    assert link.tolist() == [EM.NOLINK, 0, EM.OVER] and edits.tolist() == [0] and over.tolist() == [1]
    # q_i + k beyond the query text; a reference bound below ref_base
    assert EM.chain_edits_model(q, r, qpos, rpos, rev, pred, chain, 1, 5, ref_base=98)[0].tolist() == [EM.NOLINK, 0, EM.OVER]
    link = EM.chain_edits_model(q, r, qpos, rpos, rev, pred, chain, 1, 4, ref_base=101)[0]
    assert link[0] == EM.NOLINK and link[1] == EM.OVER and link[2] >= 0
