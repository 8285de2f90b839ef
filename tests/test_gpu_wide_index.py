"""GPU: the position index over 16-byte k-mers (WideKmerPositionIndex / kh_wide_index_*) and the position-keeping 128-bit front end
against the numpy model of tests/wide_index_model.py and the named twins, exactly (no tolerances).  The shapes follow the sort tile
(kmerhash_amd.index.SORT_TILE), the k-mer tile (4096 text positions) and the two-slot probe step of the wide table."""
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
from kmerhash_amd import wide as W  # noqa: E402
from kmerhash_amd.index import SORT_TILE as T  # noqa: E402
from index_model import fastq_masked, np_window_positions  # noqa: E402
from wide_index_model import WideIndexModel, kmers128_pos_model, pack_window128  # noqa: E402

KM_TILE = 4096      # text positions per workgroup of the k-mer front end


def dev_keys(k):
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int64)).cuda()


def distinct_wide(n, seed):
    """n distinct keys, both words random"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 63, (int(n * 1.1) + 16, 2), dtype=np.uint64)
    k = np.unique(k, axis=0)
    return rng.permutation(k)[:n]


def queries_for(keys, seed, n_miss=50):
    """hits (some repeated), misses with both words random and misses that share w0 with a hit, shuffled"""
    rng = np.random.default_rng(seed)
    u = np.unique(keys, axis=0)
    if len(u) == 0:
        return rng.integers(0, 1 << 63, (n_miss, 2), dtype=np.uint64)
    hits = u[rng.integers(0, len(u), min(len(u), 300))]
    miss = rng.integers(1 << 63, 1 << 64, (n_miss, 2), dtype=np.uint64)          # (the keys of the tests are below 2^63 in both words)
    near = hits[:20].copy()
    near[:, 1] ^= np.uint64(1 << 63)                                             # the w0 of a hit, another w1
    return rng.permutation(np.concatenate([hits, hits[:20], miss, near]))


def check_against_model(ix, keys, pos, seed=5):
    """export(), count and find (host and device queries) equal the model"""
    m = WideIndexModel(keys, pos)
    assert (ix.size(), ix.total()) == (m.size(), m.total())
    ek, eo, ep = ix.export()
    assert ek.shape == (m.size(), 2)
    mo, mp = m.export_in_key_order(ek)
    assert np.array_equal(eo, mo) and np.array_equal(ep, mp)
    assert eo[0] == 0 and eo[-1] == len(pos)
    q = queries_for(keys, seed)
    assert np.array_equal(ix.count(q), m.count(q))
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp)
    dq = dev_keys(q)
    assert np.array_equal(ix.count(dq).cpu().numpy().view(np.uint32), m.count(q))
    fo, fp = ix.find(dq)
    assert np.array_equal(fo.cpu().numpy().view(np.uint64), xo) and np.array_equal(fp.cpu().numpy().view(np.uint32), xp)
    return ek, eo, ep


@pytest.fixture
def ix():
    x = kh.WideKmerPositionIndex(k=63)
    yield x
    x.close()


# ---- build ------------------------------------------------------------------------------------------------------------------
def test_empty_build_one_pair_and_clear(ix):
    assert ix.build(np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == 0
    assert (ix.size(), ix.total(), ix.capacity()) == (0, 0, 128)
    ek, eo, ep = ix.export()
    assert len(ek) == 0 and eo.tolist() == [0] and len(ep) == 0
    q = np.array([[1, 0], [2, 2], [0, 3]], dtype=np.uint64)
    assert ix.count(q).tolist() == [0, 0, 0]
    fo, fp = ix.find(q)
    assert fo.tolist() == [0, 0, 0, 0] and len(fp) == 0
    keys, pos = np.array([[12345, 1 << 62]], dtype=np.uint64), np.array([4000000000], dtype=np.uint32)
    ix.build(keys, pos)                                         # an empty build leaves the index empty: it builds
    ek, eo, ep = check_against_model(ix, keys, pos)
    assert ek.tolist() == [[12345, 1 << 62]] and eo.tolist() == [0, 1] and ep.tolist() == [4000000000]
    with pytest.raises(kh.KhError) as e:                        # a build on a built index
        ix.build(keys, pos)
    assert e.value.status == K.KH_ERR_INVALID
    check_against_model(ix, keys, pos)                          # the refused build changed nothing
    ix.clear()
    assert (ix.size(), ix.total(), ix.capacity()) == (0, 0, 128)
    k2 = distinct_wide(500, 72)
    p2 = np.arange(500, dtype=np.uint32)
    ix.build(k2, p2)
    check_against_model(ix, k2, p2)
    fresh = kh.WideKmerPositionIndex(k=63)
    try:
        fresh.build(k2, p2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fresh.export(), ix.export())) and fresh.capacity() == ix.capacity()
    finally:
        fresh.close()


def pairs_of(keys, lens, seed):
    rng = np.random.default_rng(seed)
    k = np.repeat(np.asarray(keys, dtype=np.uint64), lens, axis=0)
    p = rng.integers(0, 1 << 32, len(k), dtype=np.uint32)
    sh = rng.permutation(len(k))
    return k[sh], p[sh]


def test_keys_of_one_home_bucket_that_differ_in_w1_only():
    """identity hash: the home bucket is w0 & (capacity - 1).  Eight keys at home 7 that differ in w1 only, three at home 8 (pushed behind
    them), four at home capacity - 1 whose run wraps the end of the table; every key with another number of positions.  Inside a run the
    exported keys ascend by (w1, w0): comparing w0 alone, moving one word only in the swap or mishandling the wrap shows here."""
    cap = 128
    ks = [(7, w1) for w1 in (5, 0, 3, 1, 7, 2, 6, 4)] + [(8, w1) for w1 in (2, 0, 1)] + [(cap - 1, w1) for w1 in (3, 1, 0, 2)]
    lens = list(range(1, len(ks) + 1))
    keys, pos = pairs_of(ks, lens, 7)
    x = kh.WideKmerPositionIndex(k=63, hash="identity")
    try:
        x.build(keys, pos)
        assert x.capacity() == cap
        ek, eo, ep = check_against_model(x, keys, pos)
        # slot order: the run of home 127 occupies slots 127, 0, 1, 2 -- its three larger keys come first, its smallest last
        want = [(cap - 1, 1), (cap - 1, 2), (cap - 1, 3)] + [(7, w1) for w1 in range(8)] + [(8, w1) for w1 in range(3)] + [(cap - 1, 0)]
        assert [tuple(r) for r in ek.tolist()] == want
        info = x.export_info()
        assert info[[127, 0, 1, 2]].tolist() == [0x80, 0x81, 0x82, 0x83]
        assert info[7:18].tolist() == [0x80 + d for d in range(8)] + [0x80 + 7, 0x80 + 8, 0x80 + 9]
        m = WideIndexModel(keys, pos)
        for key, n in zip(ks, lens):                            # find of each key alone
            fo, fp = x.find(np.array([key], dtype=np.uint64))
            xo, xp = m.find(np.array([key], dtype=np.uint64))
            assert fo.tolist() == [0, n] and np.array_equal(fp, xp)
    finally:
        x.close()


def test_odd_and_even_homes_and_probe_distances():
    """identity hash: keys at an even home (20) and an odd one (41) at probe distances 0..3, keys displaced into the middle of another
    home's run, a home that wraps (255 & 127 = 127); queried with hits and with misses that end at an empty slot, inside a run and behind
    one.  The two-slot step reads one sector on even homes and two on odd ones."""
    ks = [(20, w1) for w1 in range(4)] + [(22, 0), (22, 9)] + [(41, w1) for w1 in range(4)] + [(43, 5)] + [(127, 1), (255, 1)]
    lens = list(range(1, len(ks) + 1))
    keys, pos = pairs_of(ks, lens, 8)
    x = kh.WideKmerPositionIndex(k=63, hash="identity")
    try:
        x.build(keys, pos)
        assert x.capacity() == 128
        check_against_model(x, keys, pos)
        info = x.export_info()
        assert info[20:26].tolist() == [0x80, 0x81, 0x82, 0x83, 0x82, 0x83]       # home 22 starts at slot 24
        assert info[41:46].tolist() == [0x80, 0x81, 0x82, 0x83, 0x82]
        m = WideIndexModel(keys, pos)
        q = np.array(ks + [(20, 4), (21, 0), (22, 1), (23, 0), (24, 0), (26, 0), (40, 0), (41, 4), (42, 0), (43, 0), (45, 5), (46, 0),
                           (127, 0), (255, 0), (0, 1), (383, 1)], dtype=np.uint64)
        assert np.array_equal(x.count(q), m.count(q))
        assert m.count(q)[len(ks):].tolist() == [0] * 16
        fo, fp = x.find(dev_keys(q))
        xo, xp = m.find(q)
        assert np.array_equal(fo.cpu().numpy().view(np.uint64), xo) and np.array_equal(fp.cpu().numpy().view(np.uint32), xp)
    finally:
        x.close()


def test_one_key_longer_than_three_tiles(ix):
    n = 3 * T + 5
    pos = np.random.default_rng(3).permutation((np.arange(n, dtype=np.uint64) * 977 + 13).astype(np.uint32))
    others = distinct_wide(1001, 4)
    hot, others = others[0], others[1:]
    keys = np.concatenate([np.repeat(hot[None, :], n, axis=0), others])
    pos = np.concatenate([pos, np.arange(1000, dtype=np.uint32)])
    sh = np.random.default_rng(5).permutation(len(keys))
    keys, pos = keys[sh], pos[sh]
    ix.build(keys, pos)
    check_against_model(ix, keys, pos)
    fo, fp = ix.find(hot[None, :])
    assert fo.tolist() == [0, n] and np.array_equal(fp, np.sort(pos[(keys == hot).all(axis=1)]))


@pytest.mark.parametrize("seed", [11, 12])
def test_tile_edges(ix, seed):
    """segments of exactly T, T + 1 and T - 1 entries among singletons: whatever slot order the keys take, segments end on tile
    boundaries, straddle them and fill tiles"""
    lens = [T, T + 1, T - 1, T, 2 * T, T - 1] + [1] * 40
    keys, pos = pairs_of(distinct_wide(len(lens), seed), lens, seed)
    ix.build(keys, pos)
    ek, eo, ep = check_against_model(ix, keys, pos)
    assert (np.diff(eo.astype(np.int64)) >= T - 1).sum() == 6


def test_tile_edges_placed():
    """identity hash and keys whose w0 is their home bucket fix the slot order: a segment of T - 1 and a singleton end exactly on the first
    tile boundary, a segment of T + 1 straddles the next one, a segment of T starts off the grid and straddles the third"""
    lens = [T - 1, 1, 1, T + 1, 1, T, 1, 1]
    x = kh.WideKmerPositionIndex(k=63, hash="identity")
    try:
        ks = np.stack([np.arange(1, len(lens) + 1, dtype=np.uint64) * 3, np.arange(len(lens), dtype=np.uint64)[::-1] << np.uint64(40)], axis=1)
        keys, pos = pairs_of(ks, lens, 21)
        x.build(keys, pos)
        ek, eo, ep = check_against_model(x, keys, pos)
        assert ek.tolist() == ks.tolist()
        assert eo.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        assert eo[2] == T and eo[3] < 2 * T < eo[4] and eo[5] < 3 * T < eo[6]
    finally:
        x.close()


def skewed_pairs(seed):
    """50 000 pairs over 3 000 distinct keys, both words random: geometric multiplicities, one key above T, one key exactly once"""
    rng = np.random.default_rng(seed)
    ks = distinct_wide(3000, seed)
    w = 0.997 ** np.arange(2999)
    which = rng.choice(2999, 50_000, p=w / w.sum())
    which[:3000] = np.arange(3000)                              # every key at least once; key 2999 exactly once
    which[3000: 3000 + T + 100] = 0                             # key 0 more than T times
    keys = ks[which]
    pos = rng.integers(0, 1 << 32, 50_000, dtype=np.uint32)
    sh = rng.permutation(50_000)
    return keys[sh], pos[sh]


@pytest.mark.parametrize("hash_", ["farm", "murmur3avx64"])
def test_skew_and_determinism(hash_):
    keys, pos = skewed_pairs(31)
    m = WideIndexModel(keys, pos)
    assert m.counts.min() == 1 and m.counts.max() > T
    exports = []
    for order in (np.arange(50_000), np.random.default_rng(32).permutation(50_000)):
        x = kh.WideKmerPositionIndex(k=63, hash=hash_)
        try:
            x.build(keys[order], pos[order])
            if not exports:
                check_against_model(x, keys, pos)
            exports.append(x.export())
        finally:
            x.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(exports[0], exports[1]))


def sorted_inside_home_runs(tk, tv, home):
    """(keys (n, 2), values) in slot order with every run of equal home bucket sorted by (w1, w0); a run that wraps from the last slot to
    the first one is sorted along the ring: its tail part first, then its head part"""
    run = np.concatenate([[0], np.cumsum(home[1:] != home[:-1])])
    groups = [np.nonzero(run == r)[0] for r in range(int(run[-1]) + 1)]
    if len(groups) > 1 and home[0] == home[-1]:
        groups[-1] = np.concatenate([groups[-1], groups[0]])
        groups = groups[1:]
    ck, cv = tk.copy(), tv.copy()
    for idx in groups:
        if len(idx) > 1:
            o = np.lexsort((tk[idx, 0], tk[idx, 1]))
            ck[idx], cv[idx] = tk[idx][o], tv[idx][o]
    return ck, cv


@pytest.mark.parametrize("hash_", ["farm", "murmur3avx64"])
def test_layout_is_that_of_the_counting_twin(hash_):
    """size, capacity and info bytes equal those of a fresh hashmap_robinhood_doubling_wide after insert_reduce_plus of the same keys, the
    key sets are equal, and the exported keys are the twin's to_vector() keys with every run of one home bucket put in (w1, w0) order
    (the order inside such a run is the one freedom the counting insert leaves)"""
    keys, pos = skewed_pairs(41)
    x = kh.WideKmerPositionIndex(k=63, hash=hash_, min_load_factor=0.35, max_load_factor=0.8)
    twin = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash=hash_, seed=43)
    try:
        x.build(keys, pos)
        twin.insert_reduce_plus(keys)
        assert (x.size(), x.capacity()) == (twin.size(), twin.capacity())
        assert np.array_equal(x.export_info(), twin.export_info())
        tk, tv = twin.to_vector()
        ek, eo, _ = x.export()
        sk = lambda a: a[np.lexsort((a[:, 0], a[:, 1]))]        # noqa: E731
        assert np.array_equal(sk(ek), sk(tk))
        home = (W.hash_batch_wide(tk, hash_, 43) & np.uint64(twin.capacity() - 1)).astype(np.int64)
        canon_k, canon_v = sorted_inside_home_runs(tk, tv, home)
        assert np.array_equal(ek, canon_k)
        assert np.array_equal(np.diff(eo.astype(np.int64)), canon_v.astype(np.int64))
    finally:
        x.close()
        twin.close()


def test_k_31_agrees_with_the_64_bit_index():
    rng = np.random.default_rng(91)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 20_000)].copy()
    text[5000:9000] = text[1000:5000]                           # a repeat: keys with more than one position
    wx, nx = kh.WideKmerPositionIndex(k=31, canonical=True), kh.KmerPositionIndex(k=31, canonical=True)
    try:
        assert wx.build_sequences(text) == nx.build_sequences(text) == 20_000 - 30
        wk, _, _ = wx.export()
        nk, _, _ = nx.export()
        assert (wk[:, 1] == 0).all()
        assert np.array_equal(np.sort(wk[:, 0]), np.sort(nk))
        hits = nk[rng.integers(0, len(nk), 400)]
        q = rng.permutation(np.concatenate([hits, hits[:50], rng.integers(1 << 62, 1 << 63, 50, dtype=np.uint64)]))
        assert len(q) == 500
        wq = np.stack([q, np.zeros_like(q)], axis=1)
        no, npos = nx.find(q)
        wo, wpos = wx.find(wq)
        assert np.array_equal(no, wo) and np.array_equal(npos, wpos) and len(npos) > 450
        assert np.array_equal(nx.count(q), wx.count(wq))
    finally:
        wx.close()
        nx.close()


# ---- front end: positions next to the 16-byte k-mers --------------------------------------------------------------------------
def front_text(k):
    """2 x 4096 + k + 3 bases (windows straddle both k-mer tile boundaries) with N at 4095, 4096 and 4096 + k - 1, lower case and
    embedded newlines"""
    rng = np.random.default_rng(100 + k)
    s = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, 2 * KM_TILE + k + 3)].copy()
    s[[KM_TILE - 1, KM_TILE, KM_TILE + k - 1]] = ord("N")
    s[[100, 101 + k, 2 * KM_TILE - 2, 2 * KM_TILE + 1 + k]] = ord("\n")
    return s


_front_ref = {}


def front_ref(k, canonical):
    if (k, canonical) not in _front_ref:
        _front_ref[(k, canonical)] = kmers128_pos_model(front_text(k), k, canonical)
    return _front_ref[(k, canonical)]


@pytest.mark.parametrize("k", [1, 33, 48, 63, 64])
@pytest.mark.parametrize("canonical", [False, True])
def test_front_end_positions(k, canonical):
    text = front_text(k)
    xk, xp = front_ref(k, canonical)                                            # every (k-mer, pos) is pack_window(text, pos, k) split in words
    assert np.array_equal(xp, np_window_positions(text, k)) and len(xp) > 2 * KM_TILE - 7 * k
    if k > 1:
        assert ((xp < 2 * KM_TILE) & (xp.astype(np.int64) + k > 2 * KM_TILE)).any()     # windows that straddle a tile boundary
    plain = W.kmers128_from_sequence(text, k, canonical)
    gk, gp = W.kmers128_from_sequence(text, k, canonical, with_positions=True)
    assert gp.dtype == np.uint32 and gk.shape == (len(xp), 2)
    assert np.array_equal(gk, plain) and np.array_equal(gk, xk) and np.array_equal(gp, xp)
    dk, dp = W.kmers128_from_sequence(torch.from_numpy(text).cuda(), k, canonical, with_positions=True)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), xk) and np.array_equal(dp.cpu().numpy().view(np.uint32), xp)
    # an unaligned start: the same text at byte offset 3 of a device buffer
    buf = torch.zeros(len(text) + 3, dtype=torch.uint8, device="cuda")
    buf[3:] = torch.from_numpy(text).cuda()
    dk, dp = W.kmers128_from_sequence(buf[3:], k, canonical, with_positions=True)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), xk) and np.array_equal(dp.cpu().numpy().view(np.uint32), xp)
    # shorter than k, and exactly k
    short = text[200: 200 + k - 1]
    gk, gp = W.kmers128_from_sequence(short, k, canonical, with_positions=True) if k > 1 else (np.zeros((0, 2)), np.zeros(0))
    assert len(gk) == 0 and len(gp) == 0
    exact = text[200: 200 + k]
    gk, gp = W.kmers128_from_sequence(exact, k, canonical, with_positions=True)
    assert gp.tolist() == [0] and [tuple(r) for r in gk.tolist()] == [pack_window128(exact, 0, k, canonical)]


def small_fastq(n_reads, seed):
    """FASTQ whose id and quality lines consist of the letters ACGT"""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for _ in range(n_reads):
        ln = int(rng.integers(30, 120))
        out.append(b"@" + lut[rng.integers(0, 4, 70)].tobytes() + b"\n" + lut[rng.integers(0, 4, ln)].tobytes() + b"\n+\n"
                   + lut[rng.integers(0, 4, ln)].tobytes() + b"\n")
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy()


@pytest.mark.parametrize("k", [33, 64])
def test_front_end_positions_fastq(k):
    text = small_fastq(60, 6)
    assert len(text) > KM_TILE
    xk, xp = kmers128_pos_model(fastq_masked(text), k, True)
    assert len(xk) > 100
    plain = W.kmers128_from_fastq(text, k, True)
    gk, gp = W.kmers128_from_fastq(text, k, True, with_positions=True)
    assert np.array_equal(gk, plain) and np.array_equal(gk, xk) and np.array_equal(gp, xp)
    dk, dp = W.kmers128_from_fastq(torch.from_numpy(text).cuda(), k, True, with_positions=True)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), xk) and np.array_equal(dp.cpu().numpy().view(np.uint32), xp)


# ---- find -------------------------------------------------------------------------------------------------------------------
def test_find_misses_repeats_and_empty_batch(ix):
    keys, pos = skewed_pairs(51)
    ix.build(keys, pos)
    m = WideIndexModel(keys, pos)
    hot = m.keys[np.argmax(m.counts)]
    q = np.array([hot, (1 << 63, 1), hot, m.keys[0], (hot[0], hot[1] ^ np.uint64(1)), hot], dtype=np.uint64)
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp) and len(xp) > 3 * T
    fo, fp = ix.find(np.zeros((0, 2), dtype=np.uint64))
    assert fo.tolist() == [0] and len(fp) == 0
    fo, fp = ix.find(torch.zeros((0, 2), dtype=torch.int64, device="cuda"))
    assert fo.cpu().tolist() == [0] and len(fp) == 0
    assert len(ix.count(np.zeros((0, 2), dtype=np.uint64))) == 0
    fo, none = ix.find(q, positions=False)                      # out_pos = NULL: offsets only
    assert none is None and np.array_equal(fo, xo)


@pytest.mark.parametrize("device", [False, True])
def test_find_with_too_little_room_writes_nothing(ix, device):
    keys, pos = skewed_pairs(61)
    ix.build(keys, pos)
    m = WideIndexModel(keys, pos)
    q = np.ascontiguousarray(m.keys[:40])
    xo, xp = m.find(q)
    total = len(xp)
    L = K.lib()
    n_out = C.c_uint64()
    if device:
        dq = dev_keys(q)
        offs = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        out = torch.full((total,), -1, dtype=torch.int32, device="cuda")
        args = (dq.data_ptr(), len(q), K.KH_MEM_DEVICE, offs.data_ptr(), out.data_ptr())
    else:
        offs = np.zeros(len(q) + 1, dtype=np.uint64)
        out = np.full(total, 0xFFFFFFFF, dtype=np.uint32)
        args = (q.ctypes.data, len(q), K.KH_MEM_HOST, offs.ctypes.data, out.ctypes.data)
    assert L.kh_wide_index_find(ix._h, *args, total - 1, C.byref(n_out)) == K.KH_ERR_INVALID
    assert n_out.value == total
    got = out.cpu().numpy().view(np.uint32) if device else out
    assert (got == 0xFFFFFFFF).all()
    assert L.kh_wide_index_find(ix._h, *args, total, C.byref(n_out)) == K.KH_OK and n_out.value == total
    got = out.cpu().numpy().view(np.uint32) if device else out
    assert np.array_equal(got, xp)
    with pytest.raises(kh.KhError) as e:
        ix.find(q, cap_out=total - 1)
    assert e.value.status == K.KH_ERR_INVALID


def test_device_pairs_equal_the_host_route(ix):
    keys, pos = skewed_pairs(81)
    ix.build(dev_keys(keys), torch.from_numpy(pos.view(np.int32)).cuda())
    check_against_model(ix, keys, pos)
    host = kh.WideKmerPositionIndex(k=63)
    try:
        host.build(keys, pos)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host.export(), ix.export()))
    finally:
        host.close()


# ---- from text --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [33, 64])
def test_build_sequences_equals_build(k):
    text = front_text(k)
    gk, gp = W.kmers128_from_sequence(text, k, True, with_positions=True)
    a = kh.WideKmerPositionIndex(k=k)
    try:
        a.build(gk, gp)
        ref = a.export()
        check_against_model(a, *front_ref(k, True))
    finally:
        a.close()
    for src in (text, torch.from_numpy(text).cuda()):
        b = kh.WideKmerPositionIndex(k=k)
        try:
            assert b.build_sequences(src) == len(gp)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ref, b.export()))
        finally:
            b.close()


def test_end_to_end_fastq_k63():
    fq = KM.synthetic_fastq(200, 150, 20_000, seed=3)
    text = np.frombuffer(fq, dtype=np.uint8)
    xk, xp = kmers128_pos_model(fastq_masked(text), 63, True)
    x = kh.WideKmerPositionIndex(k=63, canonical=True)
    try:
        assert x.build_fastq(fq) == len(xk)
        check_against_model(x, xk, xp)
        q = np.unique(xk, axis=0)[::7]
        fo, fp = x.find(q)
        assert fo[-1] == len(fp) and len(fp) >= len(q)
        for i in range(len(q)):                                 # every position returned reproduces its key from the text
            for p in fp[int(fo[i]): int(fo[i + 1])].tolist():
                assert pack_window128(text, p, 63, True) == tuple(int(v) for v in q[i])
        absent = np.array([pack_window128(np.frombuffer(b"ACGT" * 16, dtype=np.uint8), 0, 63, True)], dtype=np.uint64)
        assert not (xk == absent).all(axis=1).any()
        assert x.count(absent).tolist() == [0]
    finally:
        x.close()


def test_profile_names_the_wide_kernels(ix):
    keys, pos = skewed_pairs(91)
    ix.profile_enable(True)
    ix.build(keys, pos)
    ix.find(np.ascontiguousarray(keys[:100]))
    prof = ix.profile()
    for name in ("kw_index_rank", "kw_index_scatter", "k_index_tile_sort", "k_index_seg_radix", "kw_index_lookup", "k_index_gather"):
        assert name in prof and prof[name][0] >= 1, (name, sorted(prof))
    assert not any(n in prof for n in ("k_index_rank", "k_index_scatter", "k_index_lookup"))
