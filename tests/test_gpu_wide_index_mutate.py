"""GPU: changing a built position index over 16-byte k-mers (WideKmerPositionIndex.append* / erase / erase_counts / drop_above,
kh_wide_index_*) against the numpy model of tests/wide_index_model.py, the wide counting twin (info bytes included) and the 64-bit
index at k = 31, exactly.  Keys that share w0 and differ in w1 only are part of every input."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import wide as W  # noqa: E402
from kmerhash_amd.index import SORT_TILE as T  # noqa: E402
from wide_index_model import WideIndexModel  # noqa: E402


def dev_keys(k):
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int64)).cuda()


def distinct_wide(n, seed):
    """n distinct keys, both words random; every fourth key shares its w0 with the key before it and differs in w1 only"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 63, (int(n * 1.1) + 16, 2), dtype=np.uint64)
    k = np.unique(k, axis=0)
    k = rng.permutation(k)[:n]
    k[3::4, 0] = k[2::4, 0][: len(k[3::4])]
    assert len(np.unique(k, axis=0)) == n
    return k


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


def check_against_model(ix, keys, pos, seed=5, extra_queries=None):
    """export(), count and find (host and device queries) equal the model over (keys, pos)"""
    m = WideIndexModel(keys, pos)
    assert (ix.size(), ix.total()) == (m.size(), m.total())
    ek, eo, ep = ix.export()
    assert ek.shape == (m.size(), 2)
    mo, mp = m.export_in_key_order(ek)
    assert np.array_equal(eo, mo) and np.array_equal(ep, mp)
    assert eo[0] == 0 and eo[-1] == len(pos)
    q = queries_for(keys, seed)
    if extra_queries is not None:
        q = np.concatenate([q, np.asarray(extra_queries, dtype=np.uint64).reshape(-1, 2)])
    assert np.array_equal(ix.count(q), m.count(q))
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp)
    dq = dev_keys(q)
    assert np.array_equal(ix.count(dq).cpu().numpy().view(np.uint32), m.count(q))
    fo, fp = ix.find(dq)
    assert np.array_equal(fo.cpu().numpy().view(np.uint64), xo) and np.array_equal(fp.cpu().numpy().view(np.uint32), xp)
    return ek, eo, ep


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


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


def check_layout_against_twin(x, twin, hash_, counts=True):
    """size, capacity and info bytes are the twin's; the exported keys are the twin's to_vector() keys with every home-bucket run in
    (w1, w0) order; counts: the segment lengths are the twin's values"""
    assert (x.size(), x.capacity()) == (twin.size(), twin.capacity())
    assert np.array_equal(x.export_info(), twin.export_info())
    tk, tv = twin.to_vector()
    ek, eo, _ = x.export()
    home = (W.hash_batch_wide(tk, hash_, 43) & np.uint64(twin.capacity() - 1)).astype(np.int64)
    canon_k, canon_v = sorted_inside_home_runs(tk, tv, home)
    assert np.array_equal(ek, canon_k)
    if counts:
        assert np.array_equal(np.diff(eo.astype(np.int64)), canon_v.astype(np.int64))


def new_twin(hash_="farm"):
    return kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash=hash_, seed=43)


@pytest.fixture
def ix():
    x = kh.WideKmerPositionIndex(k=63)
    yield x
    x.close()


def pairs_of(keys, lens, seed):
    rng = np.random.default_rng(seed)
    k = np.repeat(np.asarray(keys, dtype=np.uint64), lens, axis=0)
    p = rng.integers(0, 1 << 32, len(k), dtype=np.uint32)
    sh = rng.permutation(len(k))
    return k[sh], p[sh]


def skewed_pairs(seed):
    """50 000 pairs over 3 000 distinct keys: geometric multiplicities, one key above T, one key exactly once"""
    rng = np.random.default_rng(seed)
    ks = distinct_wide(3000, seed)
    w = 0.997 ** np.arange(2999)
    which = rng.choice(2999, 50_000, p=w / w.sum())
    which[:3000] = np.arange(3000)
    which[3000: 3000 + T + 100] = 0
    keys = ks[which]
    pos = rng.integers(0, 1 << 32, 50_000, dtype=np.uint32)
    sh = rng.permutation(50_000)
    return keys[sh], pos[sh]


def isin_rows(keys, rows):
    s = set(map(tuple, np.asarray(rows).tolist()))
    return np.array([tuple(r) in s for r in keys.tolist()], dtype=bool)


# ---- append -----------------------------------------------------------------------------------------------------------------
def test_append_on_an_empty_index_is_build(ix):
    keys, pos = skewed_pairs(31)
    ix.append(keys, pos)
    other = kh.WideKmerPositionIndex(k=63)
    try:
        other.build(keys, pos)
        assert same_bytes(ix.export(), other.export()) and np.array_equal(ix.export_info(), other.export_info())
    finally:
        other.close()


def test_only_new_keys_and_the_table_doubles(ix):
    ks = distinct_wide(6000, 1)
    pos = np.random.default_rng(2).integers(0, 1 << 32, 6000, dtype=np.uint32)
    twin = new_twin()
    try:
        ix.build(ks[:3000], pos[:3000])
        twin.insert_reduce_plus(ks[:3000])
        cap = ix.capacity()
        ix.append(ks[3000:], pos[3000:])
        twin.insert_reduce_plus(ks[3000:])
        assert ix.capacity() == 2 * cap
        check_against_model(ix, ks, pos)
        check_layout_against_twin(ix, twin, "farm")
    finally:
        twin.close()


@pytest.mark.parametrize("case", ["straddle", "radix", "smallest_first"])
def test_only_existing_keys(ix, case):
    """a segment of T - 1 grows by 2 and comes to straddle a tile; a segment of 1 grows by 3T + 5 (the radix path); a segment of
    3T + 5 gains one position smaller than all of its own.  The grown key has a sibling with the same w0 and another w1."""
    others = distinct_wide(42, 3)
    hot, others = others[2], np.delete(others, 2, axis=0)                     # others[3] (now [2]) shares w0 with hot
    assert others[2, 0] == hot[0] and others[2, 1] != hot[1]
    n0, n1 = {"straddle": (T - 1, 2), "radix": (1, 3 * T + 5), "smallest_first": (3 * T + 5, 1)}[case]
    rng = np.random.default_rng(4)
    p_hot = rng.permutation((np.arange(n0 + n1, dtype=np.uint64) * 977 + 1000).astype(np.uint32))
    if case == "smallest_first":
        p0, p1 = p_hot[p_hot != 1000], np.array([7], dtype=np.uint32)
    else:
        p0, p1 = p_hot[:n0], p_hot[n0:]
    k0 = np.concatenate([np.repeat(hot[None, :], len(p0), axis=0), others])
    q0 = np.concatenate([p0, np.arange(41, dtype=np.uint32)])
    sh = rng.permutation(len(k0))
    k0, q0 = k0[sh], q0[sh]
    k1 = np.repeat(hot[None, :], len(p1), axis=0)
    ix.build(k0, q0)
    ix.append(k1, p1)
    assert ix.size() == 42
    check_against_model(ix, np.concatenate([k0, k1]), np.concatenate([q0, p1]), extra_queries=[hot, others[2]])
    fo, fp = ix.find(hot[None, :])
    assert fo.tolist() == [0, len(p0) + len(p1)] and np.array_equal(fp, np.sort(np.concatenate([p0, p1])))
    fo, fp = ix.find(others[2][None, :])
    assert fo.tolist() == [0, 1]


@pytest.mark.parametrize("hash_", ["farm", "murmur3avx64"])
def test_three_batches_determinism_and_twin_layout(hash_):
    keys, pos = skewed_pairs(31)
    rng = np.random.default_rng(32)
    bounds = [0, 5_000, 12_000, 31_000, 50_000]
    batches = [(keys[a:b], pos[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    exports = []
    for permute in (False, True):
        x = kh.WideKmerPositionIndex(k=63, hash=hash_, min_load_factor=0.35, max_load_factor=0.8)
        twin = new_twin(hash_)
        try:
            for i, (bk, bp) in enumerate(batches):
                o = rng.permutation(len(bk)) if permute else np.arange(len(bk))
                (x.build if i == 0 else x.append)(bk[o], bp[o])
                twin.insert_reduce_plus(bk)
                if not permute:
                    check_layout_against_twin(x, twin, hash_)
            if not permute:
                check_against_model(x, keys, pos)
            exports.append(x.export())
        finally:
            x.close()
            twin.close()
    assert same_bytes(exports[0], exports[1])


def test_keys_of_one_home_bucket_that_differ_in_w1_only_across_batches():
    """identity hash: the home bucket is w0 & (capacity - 1).  Keys at home 7 that differ in w1 only arrive in two batches, and some
    are erased again: the runs must come out in (w1, w0) order, every key with its own positions"""
    first = [(7, w1) for w1 in (5, 0, 3)] + [(8, 2)] + [(127, 3), (127, 1)]
    second = [(7, w1) for w1 in (1, 7, 2, 6, 4)] + [(8, 0), (8, 1)] + [(127, 0), (127, 2)]
    k0, p0 = pairs_of(first, list(range(1, len(first) + 1)), 7)
    k1, p1 = pairs_of(second + first[:2], list(range(2, len(second) + 4)), 8)
    x = kh.WideKmerPositionIndex(k=63, hash="identity")
    try:
        x.build(k0, p0)
        x.append(k1, p1)
        assert x.capacity() == 128
        keys, pos = np.concatenate([k0, k1]), np.concatenate([p0, p1])
        ek, _, _ = check_against_model(x, keys, pos)
        want = [(127, 1), (127, 2), (127, 3)] + [(7, w1) for w1 in range(8)] + [(8, w1) for w1 in range(3)] + [(127, 0)]
        assert [tuple(r) for r in ek.tolist()] == want
        gone = np.array([(7, 0), (7, 4), (127, 0), (7, 9)], dtype=np.uint64)  # (7, 9) is not there: its w0 is
        m = WideIndexModel(keys, pos)
        assert x.erase(gone) == (3, int(m.count(gone).sum()))
        keep = ~isin_rows(keys, gone)
        ek, _, _ = check_against_model(x, keys[keep], pos[keep], extra_queries=gone)
        # the run of home 127 now occupies slots 127, 0, 1: its smallest key stands last in slot order
        want = [(127, 2), (127, 3)] + [(7, w1) for w1 in (1, 2, 3, 5, 6, 7)] + [(8, w1) for w1 in range(3)] + [(127, 1)]
        assert [tuple(r) for r in ek.tolist()] == want
    finally:
        x.close()


# ---- erase ------------------------------------------------------------------------------------------------------------------
def test_erase_hits_misses_repeats_and_twin(ix):
    keys, pos = skewed_pairs(41)
    twin = new_twin()
    try:
        ix.build(keys[:25_000], pos[:25_000])
        ix.append(keys[25_000:], pos[25_000:])
        twin.insert_reduce_plus(keys[:25_000])
        twin.insert_reduce_plus(keys[25_000:])
        m = WideIndexModel(keys, pos)
        u = np.unique(keys, axis=0)
        gone = u[::2]
        near = gone[:10].copy()
        near[:, 1] ^= np.uint64(1 << 63)                                      # misses that share w0 with an erased key
        batch = np.random.default_rng(42).permutation(np.concatenate([gone, near, gone[:7], gone[:1]]))
        nk, npos = ix.erase(batch)
        assert nk == len(gone) and npos == int(m.count(gone).sum())
        assert twin.erase(batch) == len(gone)
        keep = ~isin_rows(keys, gone)
        check_against_model(ix, keys[keep], pos[keep], extra_queries=gone[:40])
        check_layout_against_twin(ix, twin, "farm")
        nk, npos = ix.erase(dev_keys(u[1::2][:100]))                          # device keys
        assert nk == 100
        twin.erase(u[1::2][:100])
        check_layout_against_twin(ix, twin, "farm")
    finally:
        twin.close()


def test_erase_everything_then_append_again(ix):
    ks = distinct_wide(3000, 61)
    keys, pos = pairs_of(ks, [2] * 3000, 62)
    twin = new_twin()
    try:
        ix.build(keys, pos)
        twin.insert_reduce_plus(keys)
        cap = ix.capacity()
        assert ix.erase(ks) == (3000, 6000) and twin.erase(ks) == 3000
        assert (ix.size(), ix.total(), ix.capacity()) == (0, 0, cap) and twin.capacity() == cap      # the table keeps its capacity
        assert np.array_equal(ix.export_info(), twin.export_info())
        k2, p2 = pairs_of(ks[:50], [3] * 50, 63)
        ix.append(k2, p2)
        twin.insert_reduce_plus(k2)
        check_against_model(ix, k2, p2)
        check_layout_against_twin(ix, twin, "farm")
    finally:
        twin.close()


LENS = [1] * 40 + [2, 3, T - 1, T, T + 1, 2 * T]


def test_erase_counts_and_drop_above(ix):
    ks = distinct_wide(len(LENS), 101)
    keys, pos = pairs_of(ks, LENS, 102)
    lens = np.array(LENS)
    twin = new_twin()
    try:
        ix.build(keys, pos)
        twin.insert_reduce_plus(keys)
        before = ix.export()
        assert ix.erase_counts(4, T - 2) == (0, 0) and ix.erase_counts(3, 2) == (0, 0)      # nothing matches; lo > hi: the empty range
        assert same_bytes(before, ix.export())
        assert ix.erase_counts(2, 3) == (2, 5)
        gone = ks[(lens == 2) | (lens == 3)]
        twin.erase(gone)
        keep = ~isin_rows(keys, gone)
        check_against_model(ix, keys[keep], pos[keep], extra_queries=gone)
        check_layout_against_twin(ix, twin, "farm")
        assert ix.drop_above(T - 1) == (3, 4 * T + 1)
        gone2 = ks[lens >= T]
        twin.erase(gone2)
        keep &= ~isin_rows(keys, gone2)
        check_against_model(ix, keys[keep], pos[keep], extra_queries=gone2)
        check_layout_against_twin(ix, twin, "farm")
    finally:
        twin.close()


def test_k_31_agrees_with_the_64_bit_index_after_the_same_changes():
    rng = np.random.default_rng(91)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    t1, t2 = lut[rng.integers(0, 4, 12_000)].copy(), lut[rng.integers(0, 4, 9_000)].copy()
    t1[5000:7000] = t1[1000:3000]                                             # repeats inside the first text
    t2[2000:4000] = t1[1000:3000]                                             # and across the texts
    wx, nx = kh.WideKmerPositionIndex(k=31, canonical=True), kh.KmerPositionIndex(k=31, canonical=True)
    try:
        assert wx.build_sequences(t1) == nx.build_sequences(t1)
        assert wx.append_sequences(t2, pos_base=len(t1) + 1) == nx.append_sequences(t2, pos_base=len(t1) + 1) == 12_000 + 9_000 - 60
        nk, no, npos = nx.export()
        gone = nk[::5]
        wgone = np.stack([gone, np.zeros_like(gone)], axis=1)
        assert nx.erase(gone) == wx.erase(wgone)
        assert nx.erase_counts(3, 3) == wx.erase_counts(3, 3)
        assert nx.drop_above(1)[0] == wx.drop_above(1)[0] > 0
        assert (nx.size(), nx.total()) == (wx.size(), wx.total())
        nk, no, _ = nx.export()
        wk, _, _ = wx.export()
        # the two tables hash 8 and 16 key bytes, so their slot orders differ: the CSR is compared in ascending key order
        assert (wk[:, 1] == 0).all() and np.array_equal(np.sort(wk[:, 0]), np.sort(nk))
        q = np.concatenate([np.sort(nk), gone[:50]])
        fo, fp = nx.find(q)
        go, gp = wx.find(np.stack([q, np.zeros_like(q)], axis=1))
        assert np.array_equal(fo, go) and np.array_equal(fp, gp) and len(fp) == nx.total()
        assert int(np.diff(no.astype(np.int64)).max()) == 1
    finally:
        wx.close()
        nx.close()
