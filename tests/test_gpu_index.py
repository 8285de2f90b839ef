"""GPU: the k-mer position index (KmerPositionIndex / kh_index_*) and the position-keeping front end against the numpy model of
tests/index_model.py, exactly.  The shapes follow the sort tile the kernels use (kmerhash_amd.index.SORT_TILE): segments inside a tile,
ending on a tile boundary, straddling one, and longer than any tile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402
from kmerhash_amd.index import SORT_TILE as T  # noqa: E402
from index_model import IndexModel, np_kmers_fastq_pos, np_kmers_pos, pack_window  # noqa: E402


def distinct_keys(n, seed):
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(1, 1 << 62, int(n * 1.1) + 16, dtype=np.uint64))
    return rng.permutation(k)[:n]


def queries_for(keys, seed, n_miss=50):
    """hits (some repeated) and misses, shuffled"""
    rng = np.random.default_rng(seed)
    u = np.unique(keys)
    hits = u[rng.integers(0, len(u), min(len(u), 300))] if len(u) else np.zeros(0, dtype=np.uint64)
    miss = np.setdiff1d(rng.integers(1 << 62, 1 << 63, n_miss, dtype=np.uint64), u)
    return rng.permutation(np.concatenate([hits, hits[:20], miss]))


def check_against_model(ix, keys, pos, seed=5):
    """export(), count and find (host and device queries) equal the model"""
    m = IndexModel(keys, pos)
    assert (ix.size(), ix.total()) == (m.size(), m.total())
    ek, eo, ep = ix.export()
    mo, mp = m.export_in_key_order(ek)
    assert np.array_equal(eo, mo) and np.array_equal(ep, mp)
    assert eo[0] == 0 and eo[-1] == len(keys)
    q = queries_for(keys, seed)
    assert np.array_equal(ix.count(q), m.count(q))
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp)
    dq = torch.from_numpy(q.view(np.int64)).cuda()
    assert np.array_equal(ix.count(dq).cpu().numpy().view(np.uint32), m.count(q))
    fo, fp = ix.find(dq)
    assert np.array_equal(fo.cpu().numpy().view(np.uint64), xo) and np.array_equal(fp.cpu().numpy().view(np.uint32), xp)
    return ek, eo, ep


@pytest.fixture
def ix():
    x = kh.KmerPositionIndex(k=21)
    yield x
    x.close()


def test_empty_build(ix):
    assert ix.build(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == 0
    assert (ix.size(), ix.total()) == (0, 0)
    ek, eo, ep = ix.export()
    assert len(ek) == 0 and eo.tolist() == [0] and len(ep) == 0
    q = np.array([1, 2, 3], dtype=np.uint64)
    assert ix.count(q).tolist() == [0, 0, 0]
    fo, fp = ix.find(q)
    assert fo.tolist() == [0, 0, 0, 0] and len(fp) == 0
    ix.build(np.array([5], dtype=np.uint64), np.array([9], dtype=np.uint32))          # an empty build leaves the index empty: it builds
    assert ix.total() == 1


def test_one_pair(ix):
    keys, pos = np.array([12345], dtype=np.uint64), np.array([4000000000], dtype=np.uint32)
    ix.build(keys, pos)
    ek, eo, ep = check_against_model(ix, keys, pos)
    assert ek.tolist() == [12345] and eo.tolist() == [0, 1] and ep.tolist() == [4000000000]


def test_all_keys_distinct(ix):
    keys = distinct_keys(10_000, 1)
    pos = np.random.default_rng(2).integers(0, 1 << 32, 10_000, dtype=np.uint32)
    ix.build(keys, pos)
    check_against_model(ix, keys, pos)


@pytest.mark.parametrize("shuffled", [False, True])
def test_one_key_longer_than_three_tiles(ix, shuffled):
    n = 3 * T + 5
    pos = (np.arange(n, dtype=np.uint64) * 977 + 13).astype(np.uint32)           # ascending, spread over three byte positions
    if shuffled:
        pos = np.random.default_rng(3).permutation(pos)
    keys = np.full(n, 0x1234567890ABCDEF, dtype=np.uint64)
    ix.build(keys, pos)
    ek, eo, ep = check_against_model(ix, keys, pos)
    assert eo.tolist() == [0, n] and np.array_equal(ep, np.sort(pos))


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_tile_edges(ix, seed):
    """segments of exactly T, T + 1 and T - 1 entries among singletons: whatever slot order the keys take, segments end on tile
    boundaries, straddle them and fill tiles (three seeds: three slot orders)"""
    rng = np.random.default_rng(seed)
    lens = [T, T + 1, T - 1, T, 2 * T, T - 1] + [1] * 40
    ks = distinct_keys(len(lens), seed)
    keys = np.repeat(ks, lens)
    pos = rng.integers(0, 1 << 32, len(keys), dtype=np.uint32)
    sh = rng.permutation(len(keys))
    keys, pos = keys[sh], pos[sh]
    ix.build(keys, pos)
    ek, eo, ep = check_against_model(ix, keys, pos)
    big = eo[:-1][np.diff(eo.astype(np.int64)) >= T - 1].astype(np.int64)
    assert len(big) == 6


def test_tile_edges_placed(ix):
    """identity hash and keys that are their own home bucket fix the slot order: a segment of T - 1 and a singleton end exactly on the
    first tile boundary, a segment of T + 1 straddles the next one, a segment of T starts off the grid and straddles the third"""
    lens = [T - 1, 1, 1, T + 1, 1, T, 1, 1]
    x = kh.KmerPositionIndex(k=21, hash="identity")
    try:
        ks = np.arange(1, len(lens) + 1, dtype=np.uint64) * 3
        keys = np.repeat(ks, lens)
        rng = np.random.default_rng(21)
        pos = rng.integers(0, 1 << 20, len(keys), dtype=np.uint32)
        sh = rng.permutation(len(keys))
        x.build(keys[sh], pos[sh])
        ek, eo, ep = check_against_model(x, keys, pos)
        assert ek.tolist() == ks.tolist()                       # slot order = key order here
        assert eo.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        assert eo[2] == T and eo[3] < 2 * T < eo[4] and eo[5] < 3 * T < eo[6]
    finally:
        x.close()


def skewed_pairs(seed):
    rng = np.random.default_rng(seed)
    ks = distinct_keys(3000, seed)
    w = 0.997 ** np.arange(3000)                                # geometric multiplicities: the first keys take hundreds of positions each
    which = rng.choice(3000, 50_000, p=w / w.sum())
    which[:3000] = np.arange(3000)                              # every key at least once
    keys = ks[which]
    pos = rng.integers(0, 1 << 32, 50_000, dtype=np.uint32)
    sh = rng.permutation(50_000)
    return keys[sh], pos[sh]


def test_skewed_multiplicities_and_determinism():
    keys, pos = skewed_pairs(31)
    exports = []
    for order in (np.arange(50_000), np.arange(50_000), np.random.default_rng(32).permutation(50_000)):
        x = kh.KmerPositionIndex(k=21)
        try:
            x.build(keys[order], pos[order])
            if not exports:
                check_against_model(x, keys, pos)
            exports.append(x.export())
        finally:
            x.close()
    for e in exports[1:]:                                       # the same input twice, and a differently shuffled copy: identical bytes
        assert all(a.tobytes() == b.tobytes() for a, b in zip(exports[0], e))


def test_duplicate_pairs_are_kept(ix):
    keys = np.array([77] * 5 + [78, 79], dtype=np.uint64)
    pos = np.array([1000] * 5 + [3, 4], dtype=np.uint32)
    ix.build(keys, pos)
    check_against_model(ix, keys, pos)
    fo, fp = ix.find(np.array([77], dtype=np.uint64))
    assert fo.tolist() == [0, 5] and fp.tolist() == [1000] * 5


def sorted_inside_home_runs(tk, tv, home):
    """(keys, values) in slot order with every run of equal home bucket sorted by key; a run that wraps from the last slot to the first
    one is sorted along the ring: its tail part first, then its head part"""
    run = np.concatenate([[0], np.cumsum(home[1:] != home[:-1])])
    groups = [np.nonzero(run == r)[0] for r in range(int(run[-1]) + 1)]
    if len(groups) > 1 and home[0] == home[-1]:
        groups[-1] = np.concatenate([groups[-1], groups[0]])
        groups = groups[1:]
    ck, cv = tk.copy(), tv.copy()
    for idx in groups:
        if len(idx) > 1:
            o = np.argsort(tk[idx], kind="stable")
            ck[idx], cv[idx] = tk[idx][o], tv[idx][o]
    return ck, cv


def test_layout_is_that_of_a_counting_table():
    """Layout pin against a hashmap_robinhood_doubling twin after insert_reduce_plus of the same keys: size and capacity are equal, the
    per-key counts are the twin's values, and the keys of export() are the twin's to_vector() keys in order.

    One freedom has to be taken out of the comparison.  A Robin Hood table is sorted by home bucket, and the counting insert does not
    fix the order of the keys that SHARE a home bucket: measured on MI355X, two twins fed the same 50 000 keys (3 000 distinct) differed
    from EACH OTHER at 209 to 295 of 3 000 to_vector() places, run after run, so "equal to the twin in order" cannot hold for any index.
    The index sorts such keys ascending (its result is a function of the multiset of pairs alone); the twin's keys get the same
    treatment here -- sorted inside every run of equal home bucket, nowhere else -- and must then equal the export element by element."""
    keys, pos = skewed_pairs(41)
    for hash_ in ("farm", "murmur3avx64"):
        x = kh.KmerPositionIndex(k=21, hash=hash_, min_load_factor=0.35, max_load_factor=0.8)
        twin = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash=hash_, seed=43)
        try:
            x.build(keys, pos)
            twin.insert_reduce_plus(keys)
            assert (x.size(), x.capacity()) == (twin.size(), twin.capacity())
            tk, tv = twin.to_vector()
            ek, eo, _ = x.export()
            home = (kh.hash_batch(tk, hash_, 43) & np.uint64(twin.capacity() - 1)).astype(np.int64)
            canon_k, canon_v = sorted_inside_home_runs(tk, tv, home)
            assert np.array_equal(ek, canon_k)
            assert np.array_equal(np.diff(eo.astype(np.int64)), canon_v.astype(np.int64))
            assert (np.sort(ek) == np.sort(tk)).all()
        finally:
            x.close()
            twin.close()


def test_find_misses_repeats_and_empty_batch(ix):
    keys, pos = skewed_pairs(51)
    ix.build(keys, pos)
    m = IndexModel(keys, pos)
    hot = m.keys[np.argmax(m.counts)]
    q = np.array([hot, 1 << 63, hot, m.keys[0], (1 << 63) + 1, hot], dtype=np.uint64)
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp)
    fo, fp = ix.find(np.zeros(0, dtype=np.uint64))
    assert fo.tolist() == [0] and len(fp) == 0
    fo, fp = ix.find(torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert fo.cpu().tolist() == [0] and len(fp) == 0
    assert len(ix.count(np.zeros(0, dtype=np.uint64))) == 0
    fo, none = ix.find(q, positions=False)                      # out_pos = NULL: offsets only
    assert none is None and np.array_equal(fo, xo)


@pytest.mark.parametrize("device", [False, True])
def test_find_with_too_little_room_writes_nothing(ix, device):
    keys, pos = skewed_pairs(61)
    ix.build(keys, pos)
    m = IndexModel(keys, pos)
    q = m.keys[:40].copy()
    xo, xp = m.find(q)
    total = len(xp)
    L = K.lib()
    n_out = C.c_uint64()
    if device:
        dq = torch.from_numpy(q.view(np.int64)).cuda()
        offs = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        out = torch.full((total,), -1, dtype=torch.int32, device="cuda")
        args = (dq.data_ptr(), len(q), K.KH_MEM_DEVICE, offs.data_ptr(), out.data_ptr())
    else:
        offs = np.zeros(len(q) + 1, dtype=np.uint64)
        out = np.full(total, 0xFFFFFFFF, dtype=np.uint32)
        args = (q.ctypes.data, len(q), K.KH_MEM_HOST, offs.ctypes.data, out.ctypes.data)
    assert L.kh_index_find(ix._h, *args, total - 1, C.byref(n_out)) == K.KH_ERR_INVALID
    assert n_out.value == total
    got = out.cpu().numpy().view(np.uint32) if device else out
    assert (got == 0xFFFFFFFF).all()
    assert L.kh_index_find(ix._h, *args, total, C.byref(n_out)) == K.KH_OK and n_out.value == total
    got = out.cpu().numpy().view(np.uint32) if device else out
    assert np.array_equal(got, xp)
    with pytest.raises(kh.KhError):
        ix.find(q, cap_out=total - 1)


def test_build_twice_needs_a_clear(ix):
    k1, p1 = skewed_pairs(71)
    ix.build(k1, p1)
    with pytest.raises(kh.KhError) as e:
        ix.build(k1[:10], p1[:10])
    assert e.value.status == K.KH_ERR_INVALID
    check_against_model(ix, k1, p1)                             # the refused build changed nothing
    ix.clear()
    assert (ix.size(), ix.total(), ix.capacity()) == (0, 0, 128)
    k2 = distinct_keys(500, 72)
    p2 = np.arange(500, dtype=np.uint32)
    ix.build(k2, p2)
    check_against_model(ix, k2, p2)
    fresh = kh.KmerPositionIndex(k=21)
    try:
        fresh.build(k2, p2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fresh.export(), ix.export())) and fresh.capacity() == ix.capacity()
    finally:
        fresh.close()


def test_device_pairs(ix):
    keys, pos = skewed_pairs(81)
    ix.build(torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(pos.view(np.int32)).cuda())
    check_against_model(ix, keys, pos)


# ---- front end: positions next to the k-mers -------------------------------------------------------------------------------
def noisy_sequence(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGTNacgtn\n", dtype=np.uint8)[rng.choice(11, n, p=[.24, .24, .24, .24, .005, .005, .005, .005, .005, .005, .01])].copy()


def straddling_sequence():
    """junk up to 10 bytes before the k-mer tile boundary (4096), then a valid run of 200 bases across it, then junk: windows start in
    one tile and end in the next"""
    rng = np.random.default_rng(9)
    s = np.full(2 * 4096 + 37, ord("N"), dtype=np.uint8)
    s[4086:4286] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 200)]
    return s


def acgt_fastq(n_reads, seed):
    """FASTQ whose id and quality lines consist of the letters ACGT"""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for i in range(n_reads):
        ln = int(rng.integers(30, 90))
        out.append(b"@" + lut[rng.integers(0, 4, 12)].tobytes() + b"\n" + lut[rng.integers(0, 4, ln)].tobytes() + b"\n+\n"
                   + lut[rng.integers(0, 4, ln)].tobytes() + b"\n")
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy()


TEXTS = {"noisy": (noisy_sequence(3 * 4096 + 123, 5), False), "straddle": (straddling_sequence(), False), "fastq": (acgt_fastq(150, 6), True)}
_front_ref = {}


def front_ref(name, k, canonical):
    key = (name, k, canonical)
    if key not in _front_ref:
        text, fastq = TEXTS[name]
        _front_ref[key] = (np_kmers_fastq_pos if fastq else np_kmers_pos)(text, k, canonical)
    return _front_ref[key]


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("k", [1, 21, 31, 32])
@pytest.mark.parametrize("canonical", [False, True])
def test_front_end_positions(name, k, canonical):
    text, fastq = TEXTS[name]
    assert len(text) % 4096 != 0
    xk, xp = front_ref(name, k, canonical)
    assert len(xk) > 100
    plain = (KM.kmers_from_fastq if fastq else KM.kmers_from_sequence)(text, k, canonical)
    gk, gp = (KM.kmers_from_fastq if fastq else KM.kmers_from_sequence)(text, k, canonical, with_positions=True)
    assert np.array_equal(gk, plain) and np.array_equal(gk, xk)          # the k-mers of the existing entry point, and the model's
    assert gp.dtype == np.uint32 and np.array_equal(gp, xp)
    dk, dp = (KM.kmers_from_fastq if fastq else KM.kmers_from_sequence)(torch.from_numpy(text).cuda(), k, canonical, with_positions=True)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), xk) and np.array_equal(dp.cpu().numpy().view(np.uint32), xp)
    step = max(1, len(gp) // 200)
    for p, v in zip(gp[::step].tolist() + gp[-3:].tolist(), gk[::step].tolist() + gk[-3:].tolist()):
        assert pack_window(text, p, k, canonical) == v                   # text[p:p+k] packs to the k-mer
    if name == "straddle":
        assert ((xp < 4096) & (xp.astype(np.int64) + k > 4096)).any() or k == 1


def test_build_sequences_matches_pairs_build():
    text, _ = TEXTS["noisy"]
    xk, xp = front_ref("noisy", 21, True)
    for src in (text, torch.from_numpy(text).cuda()):
        x = kh.KmerPositionIndex(k=21, canonical=True)
        try:
            assert x.build_sequences(src) == len(xk)
            check_against_model(x, xk, xp)
        finally:
            x.close()


def test_end_to_end_fastq():
    fq = KM.synthetic_fastq(200, 150, 20_000, seed=3)
    text = np.frombuffer(fq, dtype=np.uint8)
    xk, xp = np_kmers_fastq_pos(text, 21, True)
    x = kh.KmerPositionIndex(k=21, canonical=True)
    try:
        assert x.build_fastq(fq) == len(xk)
        check_against_model(x, xk, xp)
        q = np.unique(xk)[::7]
        fo, fp = x.find(q)
        assert fo[-1] == len(fp) and len(fp) >= len(q)
        for i in range(0, len(q), 13):                                   # every position returned reproduces its key from the text
            for p in fp[int(fo[i]): int(fo[i + 1])].tolist():
                assert pack_window(text, p, 21, True) == int(q[i])
    finally:
        x.close()
