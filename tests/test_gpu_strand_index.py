"""GPU: the stranded position index, both key widths.  export() of a stranded index equals the index model over (model k-mers, np_stamp of
their positions) for every text form -- all windows, minimizers, closed syncmers, wide all windows, wide syncmers, FASTQ, an append in two
pieces with pos_base --; anchors() of a query made of a slice of the indexed text, the reverse complement of another slice and random
bases are checked one by one against the strings and as a multiset against the model; palindromes come out with rev = 0; set_stranded
on a non-empty index, canonical = 0 and a coordinate beyond 2^31 are refused with the index unchanged; and an index that is not stranded
launches exactly the kernels it launched before, a stranded one k_pos_strand once more."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from index_model import IndexModel, np_kmers_fastq_pos, np_kmers_pos  # noqa: E402
from minimizer_model import np_minimizers  # noqa: E402
from strand_model import np_stamp, np_strand_bits, revcomp_text  # noqa: E402
from syncmer_model import np_syncmers, np_syncmers_fastq  # noqa: E402
from wide_index_model import WideIndexModel, kmers128_pos_model  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
# kernel -> launches of build_sequences over `genome3k` on an index that is NOT stranded, recorded with the library of the parent commit
# (the commit before the strand bit): all windows k = 15 / closed syncmers k = 15, s = 11 / wide closed syncmers k = 63, s = 31
PARENT_PROFILES = {
    "all": {"k_build_fused": 1, "k_fused_tail": 1, "k_fused_totals": 1, "k_index_rank": 1, "k_index_scan": 1, "k_index_scatter": 1, "k_index_seg_radix": 1,
            "k_index_tile_sort": 1, "k_part_hist": 1, "k_part_scatter": 1, "k_scan": 1},
    "s11": {"k_chunk_carry": 1, "k_chunk_place": 1, "k_dedup": 1, "k_index_rank": 1, "k_index_scan": 1, "k_index_scatter": 1, "k_index_seg_radix": 1,
            "k_index_tile_sort": 1, "k_part_hist": 1, "k_part_scatter": 1, "k_scan": 2, "k_syncmers_count": 1, "k_syncmers_emit": 1},
    "wide_s31": {"k_chunk_carry": 1, "k_index_scan": 1, "k_index_seg_radix": 1, "k_index_tile_sort": 1, "k_scan": 2, "k_syncmers_count": 1, "k_syncmers_emit": 1,
                 "kw_chunk_count": 1, "kw_chunk_place": 1, "kw_dedup": 1, "kw_index_rank": 1, "kw_index_scatter": 1, "kw_part_count": 1, "kw_part_scatter": 1},
}


def random_bases(n, seed):
    return BASES[np.random.default_rng(seed).integers(0, 4, n)].copy()


@pytest.fixture(scope="module")
def genome3k():
    g = random_bases(3000, 11)
    g[400:430] |= 0x20
    g[900:960] = ord("A")
    g[1500] = ord("N")
    g[2200] = 10
    g.setflags(write=False)
    return g


def model_export_equal(ix, km, stamped, wide):
    model = (WideIndexModel if wide else IndexModel)(km, stamped)
    keys, offs, pos = ix.export()
    assert (ix.size(), ix.total()) == (model.size(), model.total())
    eo, ep = model.export_in_key_order(keys)
    assert np.array_equal(offs, eo) and np.array_equal(pos, ep)
    return model


def sampled_pairs(form, text):
    """the model's (k-mers, positions) of a text for every index form of this file: (index class, constructor arguments, pairs)"""
    if form == "all":
        return kh.KmerPositionIndex, dict(k=15), np_kmers_pos(text, 15, True), 15, False
    if form == "w5":
        return kh.KmerPositionIndex, dict(k=15, w=5), np_minimizers(text, 15, 5, True, "murmur", 42), 15, False
    if form == "s11":
        return kh.KmerPositionIndex, dict(k=15, s=11), np_syncmers(text, 15, 11, True, "murmur", 42), 15, False
    if form == "wide_all":
        return kh.WideKmerPositionIndex, dict(k=63), kmers128_pos_model(text, 63, True), 63, True
    assert form == "wide_s31"
    return kh.WideKmerPositionIndex, dict(k=63, s=31), np_syncmers(text, 63, 31, True, "murmur", 42, True), 63, True


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("form", ["all", "w5", "s11", "wide_all", "wide_s31"])
def test_export_is_the_model_over_stamped_positions(genome3k, form, where):
    cls, kwargs, (km, pos), k, wide = sampled_pairs(form, genome3k)
    stamped = np_stamp(genome3k, pos, k)
    assert len(pos) > 100 and (stamped & 1).any() and not (stamped & 1).all()
    ix = cls(stranded=True, **kwargs)
    try:
        text = np.array(genome3k) if where == "host" else torch.from_numpy(np.array(genome3k)).cuda()
        assert ix.build_sequences(text) == len(pos)
        model = model_export_equal(ix, km, stamped, wide)
        # find returns the stamped values; unstamp gives back the window positions
        offs, got = ix.find(km[:50])
        eo, ep = model.find(km[:50])
        assert np.array_equal(offs, eo) and np.array_equal(got, ep)
        p, rc = kh.unstamp(got)
        assert np.array_equal(rc, np_strand_bits(genome3k, p, k)[0])
    finally:
        ix.close()


@pytest.mark.parametrize("form", ["all", "s11", "wide_s31"])
def test_fastq_text(form):
    from kmerhash_amd.kmers import synthetic_fastq
    raw = np.frombuffer(synthetic_fastq(40, 120, genome_len=3000, seed=6), dtype=np.uint8)
    if form == "all":
        cls, kwargs, (km, pos), k, wide = kh.KmerPositionIndex, dict(k=15), np_kmers_fastq_pos(raw, 15, True), 15, False
    elif form == "s11":
        cls, kwargs, (km, pos), k, wide = kh.KmerPositionIndex, dict(k=15, s=11), np_syncmers_fastq(raw, 15, 11, True, "murmur", 42), 15, False
    else:
        cls, kwargs, (km, pos), k, wide = kh.WideKmerPositionIndex, dict(k=63, s=31), np_syncmers_fastq(raw, 63, 31, True, "murmur", 42, True), 63, True
    stamped = np_stamp(raw, pos, k)                       # (on the raw text: a window of a sequence line is k bases there too)
    assert len(pos) > 50 and (stamped != 0xFFFFFFFF).all()
    ix = cls(stranded=True, **kwargs)
    try:
        assert ix.build_fastq(raw) == len(pos)
        model_export_equal(ix, km, stamped, wide)
        ix.clear()                                          # the flag survives a clear
        assert ix.build_fastq(torch.from_numpy(np.array(raw)).cuda()) == len(pos)
        model_export_equal(ix, km, stamped, wide)
    finally:
        ix.close()


@pytest.mark.parametrize("form", ["all", "w5", "s11", "wide_s31"])
def test_append_in_two_pieces_with_pos_base(genome3k, form):
    A, B = np.array(genome3k[:1700]), random_bases(1300, 12)
    base = 1_000_000
    cls, kwargs, (ka, pa), k, wide = sampled_pairs(form, A)
    _, _, (kb, pb), _, _ = sampled_pairs(form, B)
    stamped = np.concatenate([np_stamp(A, pa, k, 7), np_stamp(B, pb, k, base)])
    ix = cls(stranded=True, **kwargs)
    try:
        ix.append_sequences(A, pos_base=7)
        assert ix.append_sequences(torch.from_numpy(B).cuda(), pos_base=base) == len(pa) + len(pb)
        model_export_equal(ix, np.concatenate([ka, kb]), stamped, wide)
    finally:
        ix.close()


def window(text, p, k):
    return bytes(text[p:p + k]).upper()


def model_anchors(ref, query, ref_pairs, query_pairs, k):
    """the anchor multiset from the model: every (query window, reference window) pair with equal canonical k-mers"""
    rk, rp = ref_pairs
    qk, qp = query_pairs
    rbit, qbit = np_strand_bits(ref, rp, k)[0], np_strand_bits(query, qp, k)[0]
    by_key = {}
    for key, p, b in zip(rk.tolist() if rk.ndim == 1 else map(tuple, rk.tolist()), rp.tolist(), rbit.tolist()):
        by_key.setdefault(key, []).append((p, b))
    out = Counter()
    for key, p, b in zip(qk.tolist() if qk.ndim == 1 else map(tuple, qk.tolist()), qp.tolist(), qbit.tolist()):
        for rpos, rb in by_key.get(key, ()):
            out[(p, rpos, b ^ rb)] += 1
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("form", ["all", "w5", "s11", "wide_s31"])
def test_anchors_are_oriented_hits(genome3k, form, where):
    T = np.array(genome3k)
    query = np.concatenate([T[500:800], revcomp_text(T[1700:2100]), random_bases(200, 13)])
    cls, kwargs, ref_pairs, k, wide = sampled_pairs(form, T)
    _, _, query_pairs, _, _ = sampled_pairs(form, query)
    ix = cls(stranded=True, **kwargs)
    try:
        ix.build_sequences(T)
        qpos, rpos, rev = ix.anchors(query if where == "host" else torch.from_numpy(query).cuda())
        if where == "device":
            assert qpos.is_cuda and rpos.is_cuda and rev.is_cuda
            qpos, rpos, rev = qpos.cpu().numpy().view(np.uint32), rpos.cpu().numpy().view(np.uint32), rev.cpu().numpy()
        assert len(qpos) == len(rpos) == len(rev) and rev.dtype == np.uint8
        # every anchor against the strings
        for q, r, v in zip(qpos.tolist(), rpos.tolist(), rev.tolist()):
            qw, rw = window(query, q, k), window(T, r, k)
            assert len(qw) == len(rw) == k
            assert rw == (qw if v == 0 else bytes(revcomp_text(np.frombuffer(qw, dtype=np.uint8)))), (q, r, v)
        # the multiset the model derives, in query order and then ascending rpos
        exp = model_anchors(T, query, ref_pairs, query_pairs, k)
        assert Counter(zip(qpos.tolist(), rpos.tolist(), rev.tolist())) == exp
        order = np.lexsort((rpos, qpos))
        assert np.array_equal(order, np.arange(len(qpos)))
        fwd = sum(c for (q, r, v), c in exp.items() if v == 0 and r == q + 500)
        back = sum(c for (q, r, v), c in exp.items() if v == 1 and q >= 300 and r == 1700 + (700 - k - q))
        assert fwd > 10 and back > 10                      # both stretches are found on their diagonal, each in its orientation
    finally:
        ix.close()


def test_anchors_of_palindromes_are_forward():
    rng = np.random.default_rng(16)
    T = random_bases(2000, 14)
    for o in (100, 700, 1300):                             # planted 16-base palindromes X + rc(X)
        x = BASES[rng.integers(0, 4, 8)]
        T[o:o + 16] = np.concatenate([x, revcomp_text(x)])
    query = np.concatenate([T[90:130], revcomp_text(T[690:730]), T[1290:1330]])
    ix = kh.KmerPositionIndex(k=16, stranded=True)
    try:
        ix.build_sequences(T)
        qpos, rpos, rev = ix.anchors(query)
        pal = [i for i, (q, r) in enumerate(zip(qpos, rpos)) if r in (100, 700, 1300) and bytes(T[r:r + 16]) == bytes(query[q:q + 16])]
        assert len(pal) >= 3 and (rev[pal] == 0).all()
        assert (rev == 1).any()                            # (the reverse-complemented stretch is there, around its palindrome)
        stamped = ix.export()[2]
        assert all(v & 1 == 0 for v in stamped if v >> 1 in (100, 700, 1300))
    finally:
        ix.close()


def test_anchors_needs_a_stranded_index(genome3k):
    for cls, kwargs in ((kh.KmerPositionIndex, dict(k=15)), (kh.WideKmerPositionIndex, dict(k=63, s=31))):
        ix = cls(**kwargs)
        try:
            ix.build_sequences(np.array(genome3k))
            with pytest.raises(ValueError, match="stranded"):
                ix.anchors(np.array(genome3k[:200]))
        finally:
            ix.close()
    w = kh.WideKmerPositionIndex(k=63, stranded=True)
    try:
        with pytest.raises(ValueError, match="without s"):
            w.anchors(np.array(genome3k[:200]))
    finally:
        w.close()


@pytest.mark.parametrize("wide", [False, True])
def test_refusals_leave_the_index_unchanged(genome3k, wide):
    L = K.lib()
    cls, pre, k = (kh.WideKmerPositionIndex, "kh_wide_index_", 63) if wide else (kh.KmerPositionIndex, "kh_index_", 15)
    g = np.array(genome3k)
    ix = cls(k=k)
    try:
        ix.build_sequences(g)
        before = [a.tobytes() for a in ix.export()]
        # set_stranded on a non-empty index
        assert getattr(L, pre + "set_stranded")(ix._h, 1) == K.KH_ERR_INVALID
        assert [a.tobytes() for a in ix.export()] == before
        ix.append_sequences(g[:100], pos_base=2 ** 32 - 200)            # (still a plain index: the 2^32 coordinate space)
        ix.clear()
        assert getattr(L, pre + "set_stranded")(ix._h, 1) == K.KH_OK    # empty: allowed
        ix.stranded = True
        ix.build_sequences(g)
        before = [a.tobytes() for a in ix.export()]
        assert (np.frombuffer(before[2], dtype=np.uint32) >> 1).max() <= len(g) - k
        # canonical == 0, pos_base + n > 2^31 and n >= 2^31 through the C ABI, every text form
        text = g.ctypes.data
        INV = K.KH_ERR_INVALID
        assert getattr(L, pre + "append_from_sequence")(ix._h, text, len(g), k, 0, K.KH_MEM_HOST, 0) == INV
        assert getattr(L, pre + "append_from_fastq")(ix._h, text, len(g), k, 0, K.KH_MEM_HOST, 0) == INV
        assert getattr(L, pre + "append_from_sequence")(ix._h, text, len(g), k, 1, K.KH_MEM_HOST, 2 ** 31 - len(g) + 1) == INV
        assert getattr(L, pre + "append_from_fastq")(ix._h, text, 1 << 31, k, 1, K.KH_MEM_HOST, 0) == INV
        assert getattr(L, pre + "append_from_syncmers")(ix._h, text, len(g), k, 11, 0, 2, 42, K.KH_MEM_HOST, 0, 0) == INV
        assert getattr(L, pre + "append_from_syncmers")(ix._h, text, len(g), k, 11, 1, 2, 42, K.KH_MEM_HOST, 0, 2 ** 31 - len(g) + 1) == INV
        if not wide:
            assert L.kh_index_append_from_minimizers(ix._h, text, len(g), k, 5, 0, 2, 42, K.KH_MEM_HOST, 0, 0) == INV
            assert L.kh_index_append_from_minimizers(ix._h, text, len(g), k, 5, 1, 2, 42, K.KH_MEM_HOST, 0, 2 ** 31 - len(g) + 1) == INV
        with pytest.raises(ValueError, match="2\\^31"):
            ix.append_sequences(g, pos_base=2 ** 31)
        assert [a.tobytes() for a in ix.export()] == before
        # the top of the coordinate space is usable
        ix.append_sequences(g[:200], pos_base=2 ** 31 - 200)
        assert ix.export()[2].max() >> 1 == 2 ** 31 - 200 + 200 - k
    finally:
        ix.close()
    # a fresh stranded index refuses canonical == 0 on a build as well
    ix = cls(k=k, stranded=True)
    try:
        assert getattr(L, pre + "build_from_sequence")(ix._h, g.ctypes.data, len(g), k, 0, K.KH_MEM_HOST) == K.KH_ERR_INVALID
        assert (ix.size(), ix.total()) == (0, 0)
        assert getattr(L, pre + "set_stranded")(ix._h, 0) == K.KH_OK
        assert getattr(L, pre + "build_from_sequence")(ix._h, g.ctypes.data, len(g), k, 0, K.KH_MEM_HOST) == K.KH_OK
    finally:
        ix.close()


def counts(prof):
    return {n: c for n, (c, _) in prof.items()}


@pytest.mark.parametrize("form", sorted(PARENT_PROFILES))
def test_kernel_profile_without_and_with_the_strand(genome3k, form):
    cls, kwargs, (km, pos), k, wide = sampled_pairs(form, genome3k)
    profs = []
    for stranded in (False, True):
        ix = cls(stranded=stranded, **kwargs)
        try:
            ix.profile_enable(True)
            assert ix.build_sequences(np.array(genome3k)) == len(pos)
            profs.append(counts(ix.profile()))
        finally:
            ix.close()
    plain, stamped = profs
    assert plain == PARENT_PROFILES[form], plain            # exactly the launches of the parent commit
    assert "k_pos_strand" not in plain and "k_anchors_expand" not in plain
    assert stamped == dict(plain, k_pos_strand=1), stamped
    # an append with pos_base: the stamp (which adds the base itself) runs once on a stranded index and never on a plain one
    if form == "all":
        for stranded in (False, True):
            ix = cls(stranded=stranded, **kwargs)
            try:
                ix.build_sequences(np.array(genome3k[:1000]))
                ix.profile_enable(True)
                ix.append_sequences(np.array(genome3k[1000:]), pos_base=5000)
                p = counts(ix.profile())
                assert p.get("k_pos_strand", 0) == (1 if stranded else 0), p
            finally:
                ix.close()
