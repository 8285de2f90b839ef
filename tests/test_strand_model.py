"""CPU: the model of the strand bit (tests/strand_model.py) against the k-mer models the suite already trusts -- the bit is 1 exactly
where the canonical k-mer differs from the forward one (oracle/kmers_np.py for k <= 32, tests/syncmer_model.np_kmers128 for k = 33..64)
-- and the properties the definition promises: palindromes give 0, the mirrored window on the reverse-complemented text has the
opposite bit, invalid windows are told apart, and stamped values sort like positions."""
import numpy as np
import pytest

from oracle.kmers_np import np_kmers
from tests.index_model import np_window_positions
from tests.strand_model import POS_INVALID, np_stamp, np_strand_bits, revcomp_text, strand_bit
from tests.syncmer_model import np_kmers128

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_text(seed, n=600):
    """bases in both cases with N, newlines, a poly-A stretch and an ACGT-repeat stretch (palindromic windows for even k)"""
    rng = np.random.default_rng(seed)
    t = BASES[rng.integers(0, 4, n)].copy()
    t[40:90] |= 0x20
    t[100:180] = ord("A")
    t[200:300] = np.frombuffer(b"ACGT" * 25, dtype=np.uint8)
    for p in rng.integers(0, n, 3):
        t[p] = ord("N")
    t[rng.integers(0, n)] = 10
    return t


@pytest.mark.parametrize("k", [1, 2, 5, 15, 16, 31, 32])
def test_bit_is_where_the_canonical_kmer_is_not_the_forward_one(k):
    t = make_text(k)
    pos = np_window_positions(t, k)
    bits, valid = np_strand_bits(t, pos, k)
    assert valid.all() and len(pos) > 300
    assert np.array_equal(bits.astype(bool), np_kmers(t, k, False) != np_kmers(t, k, True))
    assert 0 < bits.sum() < len(bits) or k == 1
    # every other position is invalid
    others = np.setdiff1d(np.arange(len(t) + 3), pos)
    assert not np_strand_bits(t, others, k)[1].any()


@pytest.mark.parametrize("k", [33, 40, 63, 64])
def test_bit_for_wide_kmers(k):
    t = make_text(100 + k)
    pos = np_window_positions(t, k)
    bits, valid = np_strand_bits(t, pos, k)
    assert valid.all() and len(pos) > 100
    assert np.array_equal(bits.astype(bool), (np_kmers128(t, k, False) != np_kmers128(t, k, True)).any(axis=1))
    assert 0 < bits.sum() < len(bits)


@pytest.mark.parametrize("k", [2, 4, 16, 32, 64])
def test_palindromes_give_zero(k):
    rng = np.random.default_rng(k)
    half = BASES[rng.integers(0, 4, k // 2)]
    pal = np.concatenate([half, revcomp_text(half)])
    assert np.array_equal(pal, revcomp_text(pal))
    assert strand_bit(pal, 0, k) == 0
    rep = np.frombuffer(b"ACGT" * 40, dtype=np.uint8)                    # ACGT repeats: half of the even-length windows are palindromes
    starts = np.arange(0, len(rep) - k + 1)
    bits, valid = np_strand_bits(rep, starts, k)
    pal_here = np.array([np.array_equal(rep[p:p + k], revcomp_text(rep[p:p + k])) for p in starts])
    assert valid.all() and pal_here.any() and (bits[pal_here] == 0).all()


@pytest.mark.parametrize("k", [1, 3, 15, 16, 33, 64])
def test_mirrored_window_has_the_opposite_bit(k):
    rng = np.random.default_rng(7 * k)
    t = BASES[rng.integers(0, 4, 400)].copy()
    if k % 2 == 0:                                             # a planted palindrome of length k (odd k has none)
        t[100:100 + k] = np.concatenate([t[100:100 + k // 2], revcomp_text(t[100:100 + k // 2])])
    r = revcomp_text(t)
    n = len(t)
    seen = 0
    for p in range(n - k + 1):
        a, b = strand_bit(t, p, k), strand_bit(r, n - k - p, k)
        if np.array_equal(t[p:p + k], revcomp_text(t[p:p + k])):
            assert a == 0 and b == 0
        else:
            assert b == 1 - a
            seen += 1
    assert seen > 300


def test_stamp_layout_and_invalid_windows():
    t = make_text(3)
    k = 15
    pos = np.array([0, 5, 5, len(t) - k, len(t) - k + 1, 0xFFFFFFFF, 101], dtype=np.uint32)
    v = np_stamp(t, pos, k, pos_base=1000)
    bits, valid = np_strand_bits(t, pos, k)
    assert v[4] == POS_INVALID and v[5] == POS_INVALID
    for i in np.nonzero(valid)[0]:
        assert v[i] >> 1 == 1000 + int(pos[i]) and v[i] & 1 == bits[i]
    assert v[1] == v[2]
    # stamped values sort like positions
    allp = np_window_positions(t, k)
    s = np_stamp(t, allp, k, 77)
    assert (np.diff(s.astype(np.int64)) > 0).all() and (s != POS_INVALID).all()
