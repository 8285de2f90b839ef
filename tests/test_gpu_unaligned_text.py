"""GPU: every entry point that reads caller text in device memory, on views at byte offsets 1, 2, 3, 4, 7, 8, 9 and 15 past a 16-byte
boundary of one allocation.  The tile loader (kh_km_pack_tile) takes one 16-byte load per lane only where the address is 16-byte
aligned and 16 byte loads padded with '\\n' otherwise; the FASTQ kernels (k_newline_tile_sums, k_fastq_mask) take 8-byte loads only at
8-byte alignment.  With an aligned base those byte branches see the tail of a text alone; here they are the whole kernel.

Expected values are those of the CPU models (oracle/kmers_np.py, tests/index_model.py, tests/minimizer_model.py, tests/syncmer_model.py,
tests/strand_model.py through tests/index_seq_model.text_pairs), never the aligned GPU run; the same bytes in a fresh aligned tensor
must give bit-identical results besides.  The bytes in front of a view are bases (FASTQ: a '\\n' and bases) and the bytes behind it are
bases: a kernel that rounded its pointer down, or read past n, would emit extra k-mers or count the lines of a FASTQ text one off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd.hll import hyperloglog64  # noqa: E402
from kmerhash_amd.index import KmerPositionIndex, WideKmerPositionIndex  # noqa: E402
from kmerhash_amd.kmers import stamp_strand  # noqa: E402
from kmerhash_amd.seqs import kmers128_from_fastq, kmers128_from_sequence, kmers_from_fastq, kmers_from_sequence  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle.kmers_np import np_kmers, np_kmers_fastq  # noqa: E402
from tests.index_seq_model import ORDER_HASH, ORDER_SEED, PairBag, text_pairs  # noqa: E402
from tests.minimizer_model import np_minimizers  # noqa: E402
from tests.strand_model import np_stamp  # noqa: E402
from tests.syncmer_model import np_syncmers  # noqa: E402

OFFSETS = (1, 2, 3, 4, 7, 8, 9, 15)
TILE = 4096                                    # start positions per workgroup of the tile loader (KH_KM_TILE)
FQ_TILE = 2048                                 # bytes per workgroup of the FASTQ newline count
BASES = b"ACGTACGTACGTACGT"
NARROW = ((1, False), (15, True), (31, True), (31, False), (32, True))          # (k, canonical)
WIDE = ((33, True), (63, True), (63, False), (64, False))


def lengths(k, o):
    """the view's end on each side of a 16-byte word, an 8-byte word and a tile, and the short texts"""
    return sorted({k - 1, k, 15, 16, 17, TILE - 1, TILE, TILE + 1, TILE + 16 - o, 8200})


def make_text(n, seed=0):
    """n bytes of ACGT with, in the last 16 bytes, a lowercase run, an N and a '\\n' (texts of 64 bytes and more; a text of 15 to 63
    bytes ends with an N or a '\\n' and has a lowercase base: the windows that do not reach its last byte stay valid), and run breaks
    on both sides of the first tile edge"""
    rng = np.random.default_rng(1000 + n + seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    if n >= 64:
        t[n - 15:n - 11] += 32                 # acgt
        t[n - 9] = ord("N")
        t[n - 4] = ord("\n")
    elif n >= 15:
        t[n - 1] = ord("N") if n % 2 else ord("\n")
        t[3] += 32
    if n > TILE + 8:
        t[TILE - 70] = ord("N")
        t[TILE + 3] = ord("\n")
    if n > 2000:
        t[700:720] += 32
    return t


def make_fastq(seed=3):
    """about 40 records with odd read lengths; the quality lines hold ACGT and @"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(40):
        ln = 61 + 2 * int(rng.integers(0, 40))
        read = bytes(rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), ln, p=[.24, .24, .24, .24, .01, .01, .005, .005, .01]))
        qual = bytes(rng.choice(np.frombuffer(b"ACGT@IIF#", dtype=np.uint8), ln))
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, read, qual))
    return np.frombuffer(b"".join(recs), dtype=np.uint8).copy()


def view_at(text, o, fastq=False):
    """-> (device view of the bytes of `text` at o bytes past a 16-byte boundary, the whole allocation).  In front: bases (FASTQ: a
    '\\n', then bases); behind: 16 bases."""
    front = ((b"\n" + BASES) if fastq else BASES)[:o]
    buf = torch.from_numpy(np.concatenate([np.frombuffer(front, dtype=np.uint8), text, np.frombuffer(BASES, dtype=np.uint8)])).cuda()
    v = buf[o:o + len(text)]
    assert buf.data_ptr() % 16 == 0 and v.numel() == len(text)
    if len(text):
        assert v.data_ptr() % 16 == o
    return v, buf


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def same_bits(a, b):
    """two results (tensors or tuples of tensors) hold the same bytes"""
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(host(x).tobytes() == host(y).tobytes() and host(x).shape == host(y).shape for x, y in zip(a, b))


def rows(km, words):
    return host(km).view(np.uint64).reshape(-1, words)


def check_front_end(fn, words, view, text, k, canonical, fastq):
    """one all-window front end on the view and on an aligned clone, with and without positions, against the model"""
    ekm, epos = text_pairs(text, k, canonical, fastq=fastq, wide=words == 2)
    if words == 1:            # the k-mer statement of the oracle itself, too
        assert np.array_equal(ekm[:, 0], (np_kmers_fastq if fastq else np_kmers)(text, k, canonical))
    clone = view.clone()
    assert clone.data_ptr() % 16 == 0
    got, ref = fn(view, k, canonical), fn(clone, k, canonical)
    assert np.array_equal(rows(got, words), ekm), (k, canonical, len(text))
    assert same_bits(got, ref)
    got, ref = fn(view, k, canonical, with_positions=True), fn(clone, k, canonical, with_positions=True)
    assert np.array_equal(rows(got[0], words), ekm) and np.array_equal(host(got[1]).view(np.uint32), epos), (k, canonical, len(text))
    assert same_bits(got, ref)
    return len(ekm)


# ---- the all-window front ends ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", OFFSETS)
def test_kmers_from_sequence_on_a_misaligned_view(o):
    total = 0
    for k, canonical in NARROW:
        for n in lengths(k, o):
            text = make_text(n)
            total += check_front_end(kmers_from_sequence, 1, view_at(text, o)[0], text, k, canonical, False)
    assert total > 5 * 2 * TILE


@pytest.mark.parametrize("o", OFFSETS)
def test_kmers128_from_sequence_on_a_misaligned_view(o):
    total = 0
    for k, canonical in WIDE:
        for n in lengths(k, o):
            text = make_text(n)
            total += check_front_end(kmers128_from_sequence, 2, view_at(text, o)[0], text, k, canonical, False)
    assert total > 4 * 2 * TILE


def newline_tile_counts(a):
    a = host(a)
    return [int((a[i:i + FQ_TILE] == 10).sum()) for i in range(0, len(a), FQ_TILE)]


@pytest.mark.parametrize("o", OFFSETS)
def test_kmers_from_fastq_on_a_misaligned_view(o):
    text = make_fastq()
    view, buf = view_at(text, o, fastq=True)
    # a kernel that rounded the pointer down would count other newlines per tile, and one more line in front of the first record
    assert newline_tile_counts(view) != newline_tile_counts(buf[:len(text)]) and len(text) > 3 * FQ_TILE
    assert host(buf[:o]).tobytes().count(b"\n") == 1
    for k, canonical in NARROW:
        assert check_front_end(kmers_from_fastq, 1, view, text, k, canonical, True) > 1000
    for k, canonical in WIDE:
        assert check_front_end(kmers128_from_fastq, 2, view, text, k, canonical, True) > 100
    # every length of the text's tail the 8-byte loads can end in: whole records cut from the front keep the end, so cut bytes of the last
    # quality line instead (the record structure stays: 4 lines per record, the last line shorter)
    for cut in range(1, 9):
        t = np.concatenate([text[:len(text) - 1 - cut], [10]]).astype(np.uint8)
        check_front_end(kmers_from_fastq, 1, view_at(t, o, fastq=True)[0], t, 15, True, True)


# ---- the strand stamp ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", OFFSETS)
def test_stamp_strand_on_a_misaligned_view(o):
    for k, n in ((15, TILE + 16 - o), (33, 8200), (64, 17), (64, 300)):
        text = make_text(n)
        view = view_at(text, o)[0]
        pos = np.concatenate([np.arange(n, dtype=np.uint32), [0, n - 1]]).astype(np.uint32)       # every start, windows past the end included
        exp = np_stamp(text, pos, k, 1000)
        dpos = torch.from_numpy(pos.view(np.int32)).cuda()
        got, ref = stamp_strand(view, dpos, k, 1000), stamp_strand(view.clone(), dpos, k, 1000)
        assert np.array_equal(host(got).view(np.uint32), exp) and same_bits(got, ref)
        assert (exp == 0xFFFFFFFF).any() and (n < 300 or (exp != 0xFFFFFFFF).sum() > n // 2)


# ---- the samplers: the offset-1 checks of tests/test_gpu_minimizers.py and tests/test_gpu_syncmers.py at every offset ----------------
@pytest.mark.parametrize("o", OFFSETS)
def test_minimizers_and_syncmers_on_a_misaligned_view(o):
    for n in (TILE + 16 - o, 8200):
        text = make_text(n)
        view = view_at(text, o)[0]
        clone = view.clone()
        for k, w, canonical in ((15, 10, True), (31, 5, False)):
            ekm, epos = np_minimizers(text, k, w, canonical, ORDER_HASH, ORDER_SEED)
            got, ref = kh.minimizers_from_sequence(view, k, w, canonical), kh.minimizers_from_sequence(clone, k, w, canonical)
            assert np.array_equal(rows(got[0], 1)[:, 0], ekm) and np.array_equal(host(got[1]).view(np.uint32), epos) and len(epos) > 100
            assert same_bits(got, ref)
        for k, s, canonical, wide in ((15, 11, True, False), (32, 8, False, False), (63, 31, True, True), (40, 20, False, True)):
            ekm, epos = np_syncmers(text, k, s, canonical, ORDER_HASH, ORDER_SEED, wide)
            fn = kh.syncmers128_from_sequence if wide else kh.syncmers_from_sequence
            got, ref = fn(view, k, s, canonical), fn(clone, k, s, canonical)
            assert np.array_equal(rows(got[0], 2 if wide else 1), np.asarray(ekm).reshape(-1, 2 if wide else 1))
            assert np.array_equal(host(got[1]).view(np.uint32), epos) and len(epos) > 100
            assert same_bits(got, ref)


# ---- the position indexes -----------------------------------------------------------------------------------------------------------
def index_bytes(x):
    return (x.size(), x.total(), x.capacity()) + tuple(a.tobytes() for a in x.export())


def same_as_bag(x, bag, query_view, query_text, sample):
    """the index against the pairs the model says it holds: sizes, the export key by key, and find_sequences of a query text"""
    m = bag.as_model()
    assert (x.size(), x.total()) == (m.size(), m.total())
    keys, off, pos = x.export()
    eo, ep = m.export_in_key_order(keys)
    assert np.array_equal(off, eo) and np.array_equal(pos, ep)
    if query_view is not None:
        qkm, qpos = text_pairs(query_text, **sample)
        eoff, ehits = m.find(qkm)
        gq, goff, ghits = x.find_sequences(query_view)
        assert np.array_equal(host(gq).view(np.uint32), qpos) and np.array_equal(host(goff).view(np.uint64), eoff)
        assert np.array_equal(host(ghits).view(np.uint32), ehits) and len(ehits) > 0
        assert same_bits((gq, goff, ghits), x.find_sequences(query_view.clone()))


INDEXES = {
    "narrow": (KmerPositionIndex, dict(k=31), dict(k=31)),
    "narrow_k15_forward": (KmerPositionIndex, dict(k=15, canonical=False), dict(k=15, canonical=False)),
    "narrow_minimizers": (KmerPositionIndex, dict(k=15, w=10), dict(k=15, w=10)),
    "narrow_syncmers": (KmerPositionIndex, dict(k=15, s=11), dict(k=15, s=11)),
    "wide": (WideKmerPositionIndex, dict(k=63), dict(k=63, wide=True)),
    "wide_syncmers": (WideKmerPositionIndex, dict(k=40, s=20), dict(k=40, s=20, wide=True)),
}


@pytest.mark.parametrize("o", OFFSETS)
@pytest.mark.parametrize("name", sorted(INDEXES))
def test_index_text_calls_on_misaligned_views(name, o):
    cls, ctor, sample = INDEXES[name]
    words = cls.WORDS
    can_query = not (words == 2 and "s" not in ctor)          # (find_sequences of 16-byte k-mers needs a sampler)
    t1, t2, fq = make_text(TILE + 16 - o), make_text(8200, seed=1), make_fastq()
    t2[100:400] = t1[50:350]                                  # shared k-mers: keys with positions from both texts
    v1, v2, vq = view_at(t1, o)[0], view_at(t2, o)[0], view_at(fq, o, fastq=True)[0]
    x, y = cls(**ctor), cls(**ctor)                           # y: the same calls on aligned clones
    bag = PairBag(words)
    # build_sequences, then append_sequences with a position base
    x.build_sequences(v1); y.build_sequences(v1.clone())
    bag.append(*text_pairs(t1, **sample))
    same_as_bag(x, bag, v2 if can_query else None, t2, sample)
    x.append_sequences(v2, pos_base=1 << 20); y.append_sequences(v2.clone(), pos_base=1 << 20)
    bag.append(*text_pairs(t2, pos_base=1 << 20, **sample))
    same_as_bag(x, bag, v1 if can_query else None, t1, sample)
    assert index_bytes(x) == index_bytes(y)
    # build_fastq on a cleared index
    x.clear(); y.clear(); bag.clear()
    x.build_fastq(vq); y.build_fastq(vq.clone())
    bag.append(*text_pairs(fq, fastq=True, **sample))
    assert bag.total() > 100
    same_as_bag(x, bag, None, None, sample)
    assert index_bytes(x) == index_bytes(y)
    x.close(); y.close()


# ---- the text-to-registers pass of HyperLogLog --------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", OFFSETS)
def test_hll_text_passes_on_a_misaligned_view(o):
    hname, hid = "murmur3avx64", O.HASH_MURMUR3_X86
    fq = make_fastq()
    vq = view_at(fq, o, fastq=True)[0]
    for k, canonical in ((15, True), (31, False), (33, True), (63, False)):
        wide = k > 32
        hashes = (O.hash16_batch if wide else O.hash_batch)
        for n in (17, TILE - 1, TILE + 16 - o, 8200):
            text = make_text(n)
            view = view_at(text, o)[0]
            km = text_pairs(text, k, canonical, wide=wide)[0]
            exp = O.OracleHLL(12, 0, hid, 43)
            if len(km):
                exp.update_via_hashval(hashes(hid, 43, np.ascontiguousarray(km if wide else km[:, 0])))
            h, g = hyperloglog64(12, 0, hname, 43), hyperloglog64(12, 0, hname, 43)
            assert h.update_from_sequence(view, k, canonical) == len(km) == g.update_from_sequence(view.clone(), k, canonical)
            assert np.array_equal(h.registers(), exp.registers()) and np.array_equal(g.registers(), exp.registers())
            h.close(); g.close()
        km = text_pairs(fq, k, canonical, fastq=True, wide=wide)[0]
        exp = O.OracleHLL(12, 0, hid, 43)
        exp.update_via_hashval(hashes(hid, 43, np.ascontiguousarray(km if wide else km[:, 0])))
        h, g = hyperloglog64(12, 0, hname, 43), hyperloglog64(12, 0, hname, 43)
        assert h.update_from_fastq(vq, k, canonical) == len(km) == g.update_from_fastq(vq.clone(), k, canonical) and len(km) > 100
        assert np.array_equal(h.registers(), exp.registers()) and np.array_equal(g.registers(), exp.registers())
        h.close(); g.close()
