"""GPU: the position index over (w,k)-minimizers (KmerPositionIndex(w=...), kh_index_build_from_minimizers / _append_from_minimizers) and
find_sequences: the export is that of a build over the pairs of minimizers_from_sequence, byte for byte, count / find agree with the
numpy models (tests/index_model.py over tests/minimizer_model.py), an append with pos_base continues the coordinate space, and the
window guarantee holds end to end -- every error-free read finds its place, on either strand.  Without w nothing changes: the same
kernels run as before."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from index_model import IndexModel  # noqa: E402
from minimizer_model import np_minimizers, np_minimizers_fastq  # noqa: E402

K_, W_ = 15, 10
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")
NEW_KERNELS = ("k_minimizers_count", "k_minimizers_emit")


def genome(n, seed):
    return BASES[np.random.default_rng(seed).integers(0, 4, n)].copy()


def queries(keys, seed):
    rng = np.random.default_rng(seed)
    u = np.unique(keys)
    hits = u[rng.integers(0, len(u), 300)]
    miss = np.setdiff1d(rng.integers(1 << 62, 1 << 63, 50, dtype=np.uint64), u)
    return rng.permutation(np.concatenate([hits, hits[:20], miss]))


def check_model(ix, keys, pos):
    m = IndexModel(keys, pos)
    assert (ix.size(), ix.total()) == (m.size(), m.total())
    ek, eo, ep = ix.export()
    mo, mp = m.export_in_key_order(ek)
    assert np.array_equal(eo, mo) and np.array_equal(ep, mp)
    q = queries(keys, 3)
    assert np.array_equal(ix.count(q), m.count(q))
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp)


@pytest.fixture(scope="module")
def g20k():
    g = genome(20_000, 21)
    g[5000:5040] = ord("A")                      # ties
    g[12_000] = ord("N")
    g[12_345] = 10
    g.setflags(write=False)
    return g, np_minimizers(g, K_, W_, True, "murmur", 42)


@pytest.mark.parametrize("where", ["host", "device"])
def test_build_sequences_is_build_over_the_minimizer_pairs(g20k, where):
    g, (ekm, epos) = g20k
    text = np.array(g) if where == "host" else torch.from_numpy(np.array(g)).cuda()
    a = kh.KmerPositionIndex(k=K_, w=W_)
    b = kh.KmerPositionIndex(k=K_, w=W_)
    try:
        a.profile_enable(True)
        assert a.build_sequences(text) == len(epos)
        prof = a.profile()
        assert all(name in prof for name in NEW_KERNELS) and "k_index_scatter" in prof, prof
        assert b.build(*kh.minimizers_from_sequence(text, K_, W_)) == len(epos)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.export(), b.export()))
        check_model(a, ekm, epos)
    finally:
        a.close(); b.close()


def test_append_with_pos_base_continues_the_coordinate_space(g20k):
    A, (akm, apos) = g20k
    B = genome(9000, 22)
    bkm, bpos = np_minimizers(B, K_, W_, True, "murmur", 42)
    ix = kh.KmerPositionIndex(k=K_, w=W_)
    try:
        ix.build_sequences(np.array(A))
        assert ix.append_sequences(torch.from_numpy(B).cuda(), pos_base=len(A)) == len(apos) + len(bpos)
        check_model(ix, np.concatenate([akm, bkm]), np.concatenate([apos, bpos + np.uint32(len(A))]))
    finally:
        ix.close()


def test_fastq_forms_and_other_order_hash():
    from kmerhash_amd.kmers import synthetic_fastq
    raw = np.frombuffer(synthetic_fastq(120, 150, genome_len=8000, seed=6), dtype=np.uint8)
    ix = kh.KmerPositionIndex(k=21, canonical=False, w=19, order_hash="farm", order_seed=7)
    try:
        ekm, epos = np_minimizers_fastq(raw, 21, 19, False, "farm", 7)
        assert ix.build_fastq(raw) == len(epos) > 0
        check_model(ix, ekm, epos)
        ix.clear()
        # whole records in two batches: split behind a record's last newline
        cut = raw.tobytes().index(b"\n@r60\n") + 1
        k1, p1 = np_minimizers_fastq(raw[:cut], 21, 19, False, "farm", 7)
        k2, p2 = np_minimizers_fastq(raw[cut:], 21, 19, False, "farm", 7)
        ix.append_fastq(raw[:cut])
        ix.append_fastq(raw[cut:], pos_base=cut)
        check_model(ix, np.concatenate([k1, k2]), np.concatenate([p1, p2 + np.uint32(cut)]))
        assert np.array_equal(np.sort(np.concatenate([p1, p2 + np.uint32(cut)])), epos)
    finally:
        ix.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_find_sequences_places_every_read(where):
    n_reads, read_len = 200, 100
    g = genome(20_000, 31)
    rng = np.random.default_rng(32)
    starts = rng.integers(0, len(g) - read_len, n_reads)
    rev = np.arange(n_reads) % 2 == 1
    ix = kh.KmerPositionIndex(k=K_, canonical=True, w=W_)
    try:
        ix.build_sequences(g)
        lines = []
        for s, r in zip(starts, rev):
            read = g[s: s + read_len]
            lines.append(COMP[read[::-1]] if r else read)
        text = np.concatenate([np.concatenate([ln, [10]]) for ln in lines]).astype(np.uint8)      # one read per line, 101 bytes each
        q = text if where == "host" else torch.from_numpy(text).cuda()
        qpos, offs, pos = ix.find_sequences(q)
        if where == "device":
            assert qpos.is_cuda and offs.is_cuda and pos.is_cuda
            qpos, offs, pos = qpos.cpu().numpy().view(np.uint32), offs.cpu().numpy().view(np.uint64), pos.cpu().numpy().view(np.uint32)
        ekm, eqpos = np_minimizers(text, K_, W_, True, "murmur", 42)
        assert np.array_equal(qpos, eqpos) and len(offs) == len(qpos) + 1
        read_of = qpos // (read_len + 1)
        in_read = (qpos % (read_len + 1)).astype(np.int64)
        placed = np.zeros(n_reads, dtype=bool)
        for i in range(len(qpos)):
            r = int(read_of[i])
            hits = pos[int(offs[i]): int(offs[i + 1])].astype(np.int64)
            want = starts[r] + read_len - in_read[i] - K_ if rev[r] else starts[r] + in_read[i]      # g + qpos + k = end | g - qpos = start
            placed[r] |= want in hits
        # an error-free read shares its w + k - 1 windows with the genome: at least one of its minimizers hits its own place
        assert placed.all(), np.nonzero(~placed)[0]
    finally:
        ix.close()


def test_find_sequences_without_w_uses_every_window():
    g = genome(3000, 41)
    ix = kh.KmerPositionIndex(k=K_)
    try:
        ix.build_sequences(g)
        qpos, offs, pos = ix.find_sequences(g[1000:1100])
        assert np.array_equal(qpos, np.arange(100 - K_ + 1, dtype=np.uint32))
        assert all(1000 + int(qpos[i]) in pos[int(offs[i]): int(offs[i + 1])] for i in range(len(qpos)))
    finally:
        ix.close()


def test_without_w_the_same_kernels_run(g20k):
    g, _ = g20k
    profs = []
    for kwargs in ({}, {"w": None, "order_hash": "farm", "order_seed": 5}):
        ix = kh.KmerPositionIndex(k=K_, **kwargs)
        try:
            ix.profile_enable(True)
            ix.build_sequences(np.array(g))
            profs.append(ix.profile())
            assert ix.total() > 19_000
        finally:
            ix.close()
    assert sorted(profs[0]) == sorted(profs[1]) and profs[0]
    assert {n: c for n, (c, _) in profs[0].items()} == {n: c for n, (c, _) in profs[1].items()}
    assert not any(n in profs[1] for n in NEW_KERNELS)


def test_wide_index_refuses_w():
    with pytest.raises(ValueError, match="16-byte"):
        kh.WideKmerPositionIndex(k=40, w=10)
    ix = kh.WideKmerPositionIndex(k=40)
    try:
        assert ix.w is None
    finally:
        ix.close()
