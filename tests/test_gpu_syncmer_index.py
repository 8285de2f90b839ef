"""GPU: the position index over closed syncmers, both key widths (KmerPositionIndex(k=15, s=11), WideKmerPositionIndex(k=40, s=20);
kh_[wide_]index_build_from_syncmers / _append_from_syncmers): build_sequences, append_sequences with pos_base and build_fastq equal an
UNSAMPLED index fed the model's pairs (tests/syncmer_model.py) through build / append -- same size, total, export, count and find --,
find_sequences looks up the model-sampled query k-mers, sampled(keys) tells "not sampled" from "absent", a refused second build changes
nothing, and without s the same kernels run as before."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from syncmer_model import kept_flags, np_kmers128, np_syncmers, np_syncmers_fastq  # noqa: E402
from oracle.kmers_np import np_kmers  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
NEW_KERNELS = ("k_syncmers_count", "k_syncmers_emit", "k_syncmer_mask")
WIDTHS = [(15, 11, False), (40, 20, True)]


def cls_of(wide):
    return kh.WideKmerPositionIndex if wide else kh.KmerPositionIndex


def genome(n, seed):
    return BASES[np.random.default_rng(seed).integers(0, 4, n)].copy()


def queries(keys, seed, wide):
    """hits (some twice) and misses, shuffled"""
    rng = np.random.default_rng(seed)
    u = np.unique(keys, axis=0)
    hits = u[rng.integers(0, len(u), 300)]
    miss = rng.integers(1 << 62, 1 << 63, (50, 2) if wide else 50, dtype=np.uint64)      # (bits no k-mer of k <= 31 / no w1 of k = 40 has)
    return rng.permutation(np.concatenate([hits, hits[:20], miss]))


def same_index(a, b, q):
    """two indexes hold the same thing: state, export, count and find CSR"""
    assert (a.size(), a.total()) == (b.size(), b.total())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.export(), b.export()))
    assert np.array_equal(a.count(q), b.count(q))
    (ao, ap), (bo, bp) = a.find(q), b.find(q)
    assert np.array_equal(ao, bo) and np.array_equal(ap, bp) and len(ap) >= 320


@pytest.fixture(scope="module")
def g20k():
    g = genome(20_000, 21)
    g[5000:5100] = ord("A")                      # ties: every window kept
    g[12_000] = ord("N")
    g[12_345] = 10
    g.setflags(write=False)
    return g, {wide: np_syncmers(g, k, s, True, "murmur", 42, wide) for k, s, wide in WIDTHS}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k,s,wide", WIDTHS)
def test_build_sequences_is_an_unsampled_build_over_the_model_pairs(g20k, k, s, wide, where):
    g, model = g20k
    ekm, epos = model[wide]
    text = np.array(g) if where == "host" else torch.from_numpy(np.array(g)).cuda()
    a, b = cls_of(wide)(k=k, s=s), cls_of(wide)(k=k)
    try:
        a.profile_enable(True)
        assert a.build_sequences(text) == len(epos) > 1500      # (20 000 bases: about 8 000 at 2/5, 1 900 at 2/21)
        prof = a.profile()
        assert "k_syncmers_count" in prof and "k_syncmers_emit" in prof and "k_index_tile_sort" in prof, prof
        assert b.build(ekm, epos) == len(epos)
        same_index(a, b, queries(ekm, 3, wide))
        # a refused second build changes nothing
        with pytest.raises(kh.KhError):
            a.build_sequences(text)
        same_index(a, b, queries(ekm, 4, wide))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("k,s,wide", WIDTHS)
def test_append_with_pos_base_continues_the_coordinate_space(g20k, k, s, wide):
    A, model = g20k
    akm, apos = model[wide]
    B = genome(9000, 22)
    bkm, bpos = np_syncmers(B, k, s, True, "murmur", 42, wide)
    a, b = cls_of(wide)(k=k, s=s), cls_of(wide)(k=k)
    try:
        a.build_sequences(np.array(A))
        assert a.append_sequences(torch.from_numpy(B).cuda(), pos_base=len(A) + 1) == len(apos) + len(bpos)
        b.build(akm, apos)
        b.append(bkm, bpos + np.uint32(len(A) + 1))
        same_index(a, b, queries(np.concatenate([akm, bkm]), 5, wide))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("k,s,wide", WIDTHS)
def test_fastq_forms_and_other_order_hash(k, s, wide):
    from kmerhash_amd.kmers import synthetic_fastq
    raw = np.frombuffer(synthetic_fastq(120, 150, genome_len=8000, seed=6), dtype=np.uint8)
    a = cls_of(wide)(k=k, canonical=False, s=s, order_hash="farm", order_seed=7)
    b = cls_of(wide)(k=k, canonical=False)
    try:
        ekm, epos = np_syncmers_fastq(raw, k, s, False, "farm", 7, wide)
        assert a.build_fastq(raw) == len(epos) > 0
        b.build(ekm, epos)
        same_index(a, b, queries(ekm, 6, wide))
        a.clear(); b.clear()
        cut = raw.tobytes().index(b"\n@r60\n") + 1       # whole records in two batches
        k1, p1 = np_syncmers_fastq(raw[:cut], k, s, False, "farm", 7, wide)
        k2, p2 = np_syncmers_fastq(raw[cut:], k, s, False, "farm", 7, wide)
        a.append_fastq(raw[:cut])
        a.append_fastq(torch.from_numpy(np.array(raw[cut:])).cuda(), pos_base=cut)
        b.append(k1, p1)
        b.append(k2, p2 + np.uint32(cut))
        same_index(a, b, queries(ekm, 7, wide))
        assert np.array_equal(np.sort(np.concatenate([p1, p2 + np.uint32(cut)])), epos)      # selection knows no neighbours: nothing lost at the cut
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k,s,wide", WIDTHS)
def test_find_sequences_looks_up_the_model_sampled_queries(g20k, k, s, wide, where):
    g, model = g20k
    ekm, epos = model[wide]
    query = np.concatenate([g[3000:3400], [10], genome(300, 77), [ord("N")], g[15_000:15_200]]).astype(np.uint8)
    qkm, eqpos = np_syncmers(query, k, s, True, "murmur", 42, wide)
    a, b = cls_of(wide)(k=k, s=s), cls_of(wide)(k=k)
    try:
        a.build_sequences(np.array(g))
        b.build(ekm, epos)
        qpos, offs, pos = a.find_sequences(query if where == "host" else torch.from_numpy(query).cuda())
        if where == "device":
            assert qpos.is_cuda and offs.is_cuda and pos.is_cuda
            qpos, offs, pos = qpos.cpu().numpy().view(np.uint32), offs.cpu().numpy().view(np.uint64), pos.cpu().numpy().view(np.uint32)
        xo, xp = b.find(qkm)
        assert np.array_equal(qpos, eqpos) and np.array_equal(offs, xo) and np.array_equal(pos, xp)
        # every syncmer of the two stretches copied from the genome finds its own place
        for i, p in enumerate(eqpos):
            if p + k <= 400:
                assert 3000 + int(p) in pos[int(offs[i]): int(offs[i + 1])]
        assert (eqpos + k <= 400).sum() > 10
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("k,s,wide", WIDTHS)
def test_sampled_separates_not_sampled_from_absent(g20k, k, s, wide):
    g, _ = g20k
    allk = np_kmers128(g, k, True) if wide else np_kmers(g, k, True)
    _, keep = kept_flags(g, k, s, True, "murmur", 42)
    other = genome(3000, 99)
    absent = np_kmers128(other, k, True) if wide else np_kmers(other, k, True)           # (random 15-mers: a few may occur in g; counted below)
    a, plain = cls_of(wide)(k=k, s=s), cls_of(wide)(k=k)
    try:
        a.build_sequences(np.array(g))
        sm, cnt = a.sampled(allk), a.count(allk)
        assert sm.dtype == bool and np.array_equal(sm, keep)
        assert (cnt[keep] > 0).all() and (cnt[~keep] == 0).all() and 0 < keep.sum() < len(keep)
        d = a.sampled(torch.from_numpy(allk.view(np.int64)).cuda())
        assert d.is_cuda and np.array_equal(d.cpu().numpy(), keep)
        # k-mers of another text: where sampled says True and count says 0 the k-mer is absent from g -- the full index agrees
        plain.build_sequences(np.array(g))
        sm2, c2, full = a.sampled(absent), a.count(absent), plain.count(absent)
        assert np.array_equal(c2 > 0, sm2 & (full > 0)) and (sm2 & (c2 == 0)).sum() > 100 and (~sm2).sum() > 100
        assert plain.sampled(absent).all() and len(plain.sampled(absent)) == len(absent)
    finally:
        a.close(); plain.close()
    w = kh.KmerPositionIndex(k=15, w=10)
    try:
        with pytest.raises(ValueError, match="minimizer"):
            w.sampled(allk[:4] if not wide else allk[:4, 0])
    finally:
        w.close()


@pytest.mark.parametrize("wide", [False, True])
def test_without_s_the_same_kernels_run(g20k, wide):
    g, _ = g20k
    k = 40 if wide else 15
    profs = []
    for kwargs in ({}, {"s": None, "order_hash": "farm", "order_seed": 5}):
        ix = cls_of(wide)(k=k, **kwargs)
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
