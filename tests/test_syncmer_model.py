"""CPU: the numpy model of closed-syncmer sampling (tests/syncmer_model.py) against a pure-Python brute force of the definition in
include/kmerhash_amd.h, one window at a time, for 8- and 16-byte k-mers, plus the properties the definition promises: s = k is the
all-window front end, exact strand symmetry, the kept fraction 2 / (k - s + 1), and the keep test on the k-mer alone."""
import numpy as np
import pytest

from tests.index_model import np_kmers_pos, pack_window
from tests.minimizer_model import order_keys
from tests.syncmer_model import kept_flags, np_is_syncmer, np_kmers128, np_syncmers, np_syncmers_fastq

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = {65: 84, 67: 71, 71: 67, 84: 65}
M64 = (1 << 64) - 1


def random_bases(rng, n):
    return BASES[rng.integers(0, 4, n)].copy()


def make_text(seed, n=400):
    """bases with N, newlines, a lower-case stretch and a poly-A stretch"""
    rng = np.random.default_rng(seed)
    t = random_bases(rng, n)
    t[40:70] |= 0x20
    t[100:190] = ord("A")
    for p in rng.integers(0, n, 3):
        t[p] = ord("N")
    for p in rng.integers(0, n, 2):
        t[p] = 10
    return t


def is_base(c):
    return chr(int(c)).upper() in "ACGT"


def brute(text, k, s, canonical, hash_id, seed):
    """the definition, one window at a time -> ([k-mer as Python int], [position])"""
    n = len(text)
    sm = {i: pack_window(text, i, s, canonical) for i in range(n - s + 1) if all(is_base(text[i + j]) for j in range(s))}
    order = sorted(sm)
    h = dict(zip(order, (int(x) for x in order_keys(np.array([sm[i] for i in order], dtype=np.uint64), hash_id, seed))))
    kms, pos = [], []
    for p in range(n - k + 1):
        if not all(is_base(text[p + j]) for j in range(k)):
            continue
        keys = [h[i] for i in range(p, p + k - s + 1)]
        if keys[0] == min(keys) or keys[-1] == min(keys):
            kms.append(pack_window(text, p, k, canonical)); pos.append(p)
    return kms, pos


def rows(kms):
    return np.array([(v & M64, v >> 64) for v in kms], dtype=np.uint64).reshape(-1, 2)


CASES = [(15, 11, True, "murmur", 42), (9, 9, False, "farm", 7), (7, 1, True, "murmur3avx64", 1), (12, 5, False, "identity", 0),
         (32, 21, True, "farm", 3), (33, 32, True, "murmur", 42), (64, 32, False, "farm", 9), (40, 20, True, "murmur", 42),
         (64, 1, True, "murmur", 5), (20, 7, True, "farm", 1)]


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("k,s,canonical,hash_id,hseed", CASES)
def test_model_equals_brute_force(seed, k, s, canonical, hash_id, hseed):
    text = make_text(seed)
    bkm, bpos = brute(text, k, s, canonical, hash_id, hseed)
    assert len(bpos) > 0
    if k <= 32:
        km, pos = np_syncmers(text, k, s, canonical, hash_id, hseed)
        assert km.dtype == np.uint64 and pos.dtype == np.uint32
        assert np.array_equal(pos, np.array(bpos, dtype=np.uint32)) and np.array_equal(km, np.array(bkm, dtype=np.uint64))
    km, pos = np_syncmers(text, k, s, canonical, hash_id, hseed, wide=True)
    assert km.shape == (len(bpos), 2) and np.array_equal(pos, np.array(bpos, dtype=np.uint32)) and np.array_equal(km, rows(bkm))


def test_fastq_form_masks_ids_and_qualities():
    from kmerhash_amd.kmers import synthetic_fastq
    raw = synthetic_fastq(6, 60, genome_len=2000, seed=4).replace(b"I", b"A")
    text = np.frombuffer(raw, dtype=np.uint8)
    for k, s, wide in ((9, 5, False), (40, 20, True)):
        km, pos = np_syncmers_fastq(text, k, s, True, "murmur", 42, wide)
        assert len(km)
        line = np.concatenate([[0], np.cumsum(text == 10)[:-1]])
        assert (line[pos] % 4 == 1).all() and (line[pos + k - 1] == line[pos]).all()
        # the same reads as plain sequence lines, one per line: the same k-mers
        seqs = b"\n".join(raw.split(b"\n")[1::4]) + b"\n"
        km2, _ = np_syncmers(np.frombuffer(seqs, dtype=np.uint8), k, s, True, "murmur", 42, wide)
        assert np.array_equal(km, km2)


@pytest.mark.parametrize("k,canonical", [(1, False), (15, True), (32, True)])
def test_s_equal_k_is_every_window(k, canonical):
    text = make_text(5)
    km, pos = np_syncmers(text, k, k, canonical, "murmur", 42)
    ekm, epos = np_kmers_pos(text, k, canonical)
    assert np.array_equal(km, ekm) and np.array_equal(pos, epos)
    km2, pos2 = np_syncmers(text, k, k, canonical, "murmur", 42, wide=True)
    assert np.array_equal(pos2, epos) and np.array_equal(km2[:, 0], ekm) and not km2[:, 1].any()


def test_s1_keeps_the_k_mers_whose_end_base_is_a_smallest_one():
    text = make_text(6)
    _, pos = np_syncmers(text, 15, 1, False, "identity", 0)                # identity order: A < C < G < T
    code = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
    for p in np_kmers_pos(text, 15, False)[1]:
        w = [code[int(c)] for c in text[p: p + 15]]
        assert (int(p) in pos) == (min(w) in (w[0], w[-1]))


def test_poly_a_keeps_every_window():
    text = np.frombuffer(b"N" + b"A" * 80 + b"N", dtype=np.uint8)
    for k, s, wide in ((15, 11, False), (40, 20, True)):
        _, pos = np_syncmers(text, k, s, True, "murmur", 42, wide)
        assert np.array_equal(pos, np.arange(1, 1 + 80 - k + 1, dtype=np.uint32))


def test_text_shorter_than_k_and_runs_of_exactly_k():
    rng = np.random.default_rng(3)
    for k, s, wide in ((15, 11, False), (63, 31, True)):
        for n in (0, 1, k - 1):
            km, pos = np_syncmers(random_bases(rng, n), k, s, True, "murmur", 42, wide)
            assert len(km) == 0 and len(pos) == 0
        # a run of exactly k bases yields its k-mer iff that k-mer is a syncmer: selection needs no neighbours
        kept = 0
        for _ in range(40):
            run = random_bases(rng, k)
            text = np.concatenate([[ord("N")], run, [10]]).astype(np.uint8)
            km, pos = np_syncmers(text, k, s, True, "murmur", 42, wide)
            full = np_kmers128(run, k, True) if wide else np_kmers_pos(run, k, True)[0]
            assert len(km) == int(np_is_syncmer(full, k, s, True, "murmur", 42)[0]) and (len(pos) == 0 or pos[0] == 1)
            kept += len(km)
        assert 0 < kept < 40


def revcomp(t):
    return np.array([COMP[int(c)] for c in t[::-1]], dtype=np.uint8)


@pytest.mark.parametrize("k,s,wide", [(15, 11, False), (31, 21, False), (7, 1, False), (63, 31, True), (40, 20, True), (64, 32, True)])
@pytest.mark.parametrize("hash_id", ["murmur", "farm"])
def test_strand_symmetry(k, s, wide, hash_id):
    rng = np.random.default_rng(100 + k)
    t = random_bases(rng, 3000)
    t[500:600] = ord("A")
    n = len(t)
    ka, pa = np_syncmers(t, k, s, True, hash_id, 42, wide)
    kb, pb = np_syncmers(revcomp(t), k, s, True, hash_id, 42, wide)
    mirrored = (n - k - pb.astype(np.int64))[::-1]
    assert np.array_equal(pa.astype(np.int64), mirrored) and np.array_equal(ka, kb[::-1])


@pytest.mark.parametrize("k,s", [(15, 11), (31, 21), (63, 31)])
def test_kept_fraction(k, s):
    """within 3 % (relative) of 2 / (k - s + 1) on 2e5 random bases"""
    t = random_bases(np.random.default_rng(2021), 200_000)
    pos, keep = kept_flags(t, k, s, True, "murmur", 42)
    frac, want = keep.mean(), 2.0 / (k - s + 1)
    print("k=%d s=%d kept %.5f expected %.5f" % (k, s, frac, want))
    assert len(pos) == len(t) - k + 1 and abs(frac - want) <= 0.03 * want


@pytest.mark.parametrize("k,s,canonical,hash_id", [(15, 11, True, "murmur"), (15, 1, False, "farm"), (32, 32, True, "murmur"), (31, 21, False, "murmur3avx64"),
                                                   (63, 31, True, "murmur"), (64, 1, True, "farm"), (40, 20, False, "identity")])
def test_is_syncmer_equals_the_kept_flag_of_every_window(k, s, canonical, hash_id):
    text = make_text(7, 600)
    pos, keep = kept_flags(text, k, s, canonical, hash_id, 42)
    km = np_kmers128(text, k, canonical)
    assert len(km) == len(pos) > 100
    assert np.array_equal(np_is_syncmer(km, k, s, canonical, hash_id, 42), keep)
    if k <= 32:
        assert np.array_equal(np_is_syncmer(np_kmers_pos(text, k, canonical)[0], k, s, canonical, hash_id, 42), keep)
    if canonical:      # a canonical key and the other strand's bit pattern agree
        fw = np_kmers128(text, k, False)
        assert np.array_equal(np_is_syncmer(fw, k, s, True, hash_id, 42), keep)
