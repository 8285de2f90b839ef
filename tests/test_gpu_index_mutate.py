"""GPU: changing a built position index (KmerPositionIndex.append* / erase / erase_counts / drop_above, kh_index_*) against the numpy
model of tests/index_model.py over the pairs that should be in the index, exactly, and against a counting twin fed the same batches.
The shapes follow the sort tile (kmerhash_amd.index.SORT_TILE): segments that grow across a tile boundary, onto the radix path, and
the smallest table at which an insert doubles the capacity between two batches."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from kmerhash_amd.index import SORT_TILE as T  # noqa: E402
from index_model import IndexModel, np_kmers_fastq_pos, np_kmers_pos  # noqa: E402
from oracle import oracle_py as O  # noqa: E402


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


def dev(a, dt=np.int64):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()


def check_against_model(ix, keys, pos, seed=5, extra_queries=None):
    """export(), count and find (host and device queries) equal the model over (keys, pos)"""
    m = IndexModel(keys, pos)
    assert (ix.size(), ix.total()) == (m.size(), m.total())
    ek, eo, ep = ix.export()
    mo, mp = m.export_in_key_order(ek)
    assert np.array_equal(eo, mo) and np.array_equal(ep, mp)
    assert eo[0] == 0 and eo[-1] == len(keys)
    q = queries_for(keys, seed)
    if extra_queries is not None:
        q = np.concatenate([q, np.asarray(extra_queries, dtype=np.uint64)])
    assert np.array_equal(ix.count(q), m.count(q))
    fo, fp = ix.find(q)
    xo, xp = m.find(q)
    assert np.array_equal(fo, xo) and np.array_equal(fp, xp)
    dq = dev(q)
    assert np.array_equal(ix.count(dq).cpu().numpy().view(np.uint32), m.count(q))
    fo, fp = ix.find(dq)
    assert np.array_equal(fo.cpu().numpy().view(np.uint64), xo) and np.array_equal(fp.cpu().numpy().view(np.uint32), xp)
    return ek, eo, ep


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


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


def check_layout_against_twin(x, twin, hash_, counts=True):
    """size, capacity, and the exported keys = the twin's to_vector() keys with every home-bucket run in key order; counts: the segment
    lengths are the twin's values"""
    assert (x.size(), x.capacity()) == (twin.size(), twin.capacity())
    tk, tv = twin.to_vector()
    ek, eo, _ = x.export()
    home = (kh.hash_batch(tk, hash_, 43) & np.uint64(twin.capacity() - 1)).astype(np.int64)
    canon_k, canon_v = sorted_inside_home_runs(tk, tv, home)
    assert np.array_equal(ek, canon_k)
    if counts:
        assert np.array_equal(np.diff(eo.astype(np.int64)), canon_v.astype(np.int64))


@pytest.fixture
def ix():
    x = kh.KmerPositionIndex(k=21)
    yield x
    x.close()


def pairs_of(ks, lens, seed, hi=1 << 32):
    rng = np.random.default_rng(seed)
    keys = np.repeat(np.asarray(ks, dtype=np.uint64), lens)
    pos = rng.integers(0, hi, len(keys), dtype=np.uint32)
    sh = rng.permutation(len(keys))
    return keys[sh], pos[sh]


def skewed_pairs(seed):
    """the skewed input of test_gpu_index.py: 50 000 pairs over 3 000 keys, geometric multiplicities"""
    rng = np.random.default_rng(seed)
    ks = distinct_keys(3000, seed)
    w = 0.997 ** np.arange(3000)
    which = rng.choice(3000, 50_000, p=w / w.sum())
    which[:3000] = np.arange(3000)
    keys = ks[which]
    pos = rng.integers(0, 1 << 32, 50_000, dtype=np.uint32)
    sh = rng.permutation(50_000)
    return keys[sh], pos[sh]


# ---- append -----------------------------------------------------------------------------------------------------------------
def test_append_on_an_empty_index_is_build(ix):
    keys, pos = skewed_pairs(31)
    assert ix.append(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)) == 0
    assert (ix.size(), ix.total(), ix.capacity()) == (0, 0, 128)
    assert ix.append(keys, pos) == len(keys)
    other = kh.KmerPositionIndex(k=21)
    try:
        other.build(keys, pos)
        assert same_bytes(ix.export(), other.export()) and ix.capacity() == other.capacity()
    finally:
        other.close()
    check_against_model(ix, keys, pos)


def test_only_new_keys_and_the_table_doubles(ix):
    ks = distinct_keys(6000, 1)
    pos = np.random.default_rng(2).integers(0, 1 << 32, 6000, dtype=np.uint32)
    ix.build(ks[:3000], pos[:3000])
    cap = ix.capacity()
    check_against_model(ix, ks[:3000], pos[:3000])
    ix.append(ks[3000:], pos[3000:])
    assert ix.capacity() == 2 * cap
    check_against_model(ix, ks, pos)


@pytest.mark.parametrize("case", ["straddle", "radix", "smallest_first"])
def test_only_existing_keys(ix, case):
    """a segment of T - 1 grows by 2 and comes to straddle a tile; a segment of 1 grows by 3T + 5 (the radix path); a segment of
    3T + 5 gains one position smaller than all of its own, which must come out first"""
    others = distinct_keys(41, 3)
    hot, others = others[0], others[1:]
    n0, n1 = {"straddle": (T - 1, 2), "radix": (1, 3 * T + 5), "smallest_first": (3 * T + 5, 1)}[case]
    rng = np.random.default_rng(4)
    p_hot = rng.permutation((np.arange(n0 + n1, dtype=np.uint64) * 977 + 1000).astype(np.uint32))
    if case == "smallest_first":
        p0, p1 = p_hot[p_hot != 1000], np.array([7], dtype=np.uint32)      # 7 is below every position the segment holds
    else:
        p0, p1 = p_hot[:n0], p_hot[n0:]
    k0 = np.concatenate([np.full(len(p0), hot, dtype=np.uint64), others])
    q0 = np.concatenate([p0, np.arange(40, dtype=np.uint32)])
    sh = rng.permutation(len(k0))
    k0, q0 = k0[sh], q0[sh]
    k1 = np.full(len(p1), hot, dtype=np.uint64)
    ix.build(k0, q0)
    size = ix.size()
    ix.append(k1, p1)
    assert ix.size() == size
    allk, allp = np.concatenate([k0, k1]), np.concatenate([q0, p1])
    check_against_model(ix, allk, allp, extra_queries=[hot])
    fo, fp = ix.find(np.array([hot], dtype=np.uint64))
    assert fo.tolist() == [0, len(p0) + len(p1)] and np.array_equal(fp, np.sort(np.concatenate([p0, p1])))
    if case == "smallest_first":
        assert fp[0] == 7


def test_new_positions_interleave_and_a_present_pair_is_kept_twice(ix):
    k0 = np.array([77] * 4 + [78, 79], dtype=np.uint64)
    p0 = np.array([10, 30, 50, 70, 3, 4], dtype=np.uint32)
    k1 = np.array([77, 77, 77, 80, 78], dtype=np.uint64)
    p1 = np.array([40, 20, 30, 9, 3], dtype=np.uint32)                       # (77, 30) and (78, 3) are in the index already
    ix.build(k0, p0)
    ix.append(k1, p1)
    check_against_model(ix, np.concatenate([k0, k1]), np.concatenate([p0, p1]))
    fo, fp = ix.find(np.array([77, 78, 80], dtype=np.uint64))
    assert fo.tolist() == [0, 7, 9, 10] and fp.tolist() == [10, 20, 30, 30, 40, 50, 70, 3, 3, 9]


@pytest.mark.parametrize("hash_", ["farm", "murmur3avx64"])
def test_batches_determinism_and_twin_layout(hash_):
    """the skewed input split 20 000 / 30 000, and three appends in a row on a further split: permuting the pairs inside each batch
    changes no byte of the export, and the layout is the twin's after insert_reduce_plus of the same batches"""
    keys, pos = skewed_pairs(31)
    rng = np.random.default_rng(32)
    for cuts in ([20_000], [5_000, 12_000, 31_000]):
        bounds = [0] + cuts + [50_000]
        batches = [(keys[a:b], pos[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
        exports = []
        for permute in (False, True):
            x = kh.KmerPositionIndex(k=21, hash=hash_, min_load_factor=0.35, max_load_factor=0.8)
            twin = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash=hash_, seed=43)
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


def test_one_shot_equality():
    """where the twin's capacity after two inserts equals the capacity of one insert of the concatenation, build + append exports the
    bytes of the one-shot build.  The split is found with the CPU oracle before anything runs on the GPU."""
    keys, pos = skewed_pairs(31)
    zeros = lambda n: np.zeros(n, dtype=np.uint32)                            # noqa: E731
    one = O.OracleTable(O.KIND_RH, 128, 0.35, 0.8, O.HASH_FARM, 43)
    one.insert(keys, zeros(len(keys)))
    cut = None
    for c in (40_000, 30_000, 20_000, 10_000, 45_000, 49_000):
        two = O.OracleTable(O.KIND_RH, 128, 0.35, 0.8, O.HASH_FARM, 43)
        two.insert(keys[:c], zeros(c))
        two.insert(keys[c:], zeros(len(keys) - c))
        if two.capacity() == one.capacity() and two.size() == one.size():
            cut = c
            break
    assert cut is not None, "no split of the input keeps the one-shot capacity"
    a, b = kh.KmerPositionIndex(k=21), kh.KmerPositionIndex(k=21)
    t1 = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43)
    t2 = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43)
    try:
        t1.insert_reduce_plus(keys)
        t2.insert_reduce_plus(keys[:cut])
        t2.insert_reduce_plus(keys[cut:])
        assert t1.capacity() == t2.capacity() == one.capacity()
        a.build(keys, pos)
        b.build(keys[:cut], pos[:cut])
        b.append(keys[cut:], pos[cut:])
        assert a.capacity() == b.capacity() == t1.capacity()
        ea, eb = a.export(), b.export()
        assert ea[0].tobytes() == eb[0].tobytes() and ea[1].tobytes() == eb[1].tobytes() and ea[2].tobytes() == eb[2].tobytes()
    finally:
        for o in (a, b, t1, t2):
            o.close()


def test_device_pairs_for_append_and_erase(ix):
    keys, pos = skewed_pairs(81)
    ix.build(dev(keys[:20_000]), dev(pos[:20_000], np.int32))
    ix.append(dev(keys[20_000:]), dev(pos[20_000:], np.int32))
    check_against_model(ix, keys, pos)
    gone = np.unique(keys)[::3]
    m = IndexModel(keys, pos)
    nk, npos = ix.erase(dev(np.concatenate([gone, gone[:5]])))
    assert (nk, npos) == (len(gone), int(m.count(gone).sum()))
    keep = ~np.isin(keys, gone)
    check_against_model(ix, keys[keep], pos[keep], extra_queries=gone[:30])


def text_of(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.choice(9, n, p=[.24, .24, .24, .24, .01, .0075, .0075, .0075, .0075])].copy()


def fastq_of(n_reads, seed):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for _ in range(n_reads):
        ln = int(rng.integers(30, 90))
        out.append(b"@" + lut[rng.integers(0, 4, 12)].tobytes() + b"\n" + lut[rng.integers(0, 4, ln)].tobytes() + b"\n+\n"
                   + lut[rng.integers(0, 4, ln)].tobytes() + b"\n")
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy()


@pytest.mark.parametrize("on_device", [False, True])
def test_append_sequences_in_one_coordinate_space(ix, on_device):
    first, second = text_of(4096 + 77, 5), text_of(2 * 4096 + 11, 6)
    second[100:600] = first[200:700]                                          # shared k-mers: segments with positions from both texts
    whole = np.concatenate([first, np.frombuffer(b"\n", dtype=np.uint8), second])
    xk, xp = np_kmers_pos(whole, 21, True)
    put = (lambda a: torch.from_numpy(a).cuda()) if on_device else (lambda a: a)
    n1 = ix.append_sequences(put(first))
    assert n1 == len(np_kmers_pos(first, 21, True)[0])
    assert ix.append_sequences(put(second), pos_base=len(first) + 1) == len(xk)
    check_against_model(ix, xk, xp)


def test_append_fastq_in_one_coordinate_space(ix):
    first, second = fastq_of(60, 7), fastq_of(90, 8)
    whole = np.concatenate([first, second])                                   # whole records: the second text starts on a record boundary
    xk, xp = np_kmers_fastq_pos(whole, 21, True)
    ix.build_fastq(first)
    assert ix.append_fastq(second.tobytes(), pos_base=len(first)) == len(xk)
    check_against_model(ix, xk, xp)


def test_refused_appends_leave_the_index_unchanged(ix):
    keys, pos = skewed_pairs(71)
    ix.build(keys, pos)
    before = ix.export()
    with pytest.raises(kh.KhError) as e:                                      # a window position would wrap
        ix.append_sequences(text_of(100, 9)[:100], pos_base=2 ** 32 - 1)
    assert e.value.status == K.KH_ERR_INVALID
    assert same_bytes(before, ix.export())
    with pytest.raises(ValueError):
        ix.append(keys[:10], pos[:9])
    with pytest.raises(ValueError):
        ix.append(keys[:10], dev(pos[:10], np.int32))
    assert same_bytes(before, ix.export())
    assert ix.append_sequences(text_of(100, 9), pos_base=2 ** 32 - 100) > len(keys)      # the last position that fits is taken
    assert int(ix.export()[2].max()) <= 2 ** 32 - 21


# ---- erase ------------------------------------------------------------------------------------------------------------------
def test_erase_hits_misses_repeats_and_twin(ix):
    keys, pos = skewed_pairs(41)
    twin = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43)
    try:
        ix.build(keys, pos)
        twin.insert_reduce_plus(keys)
        m = IndexModel(keys, pos)
        u = np.unique(keys)
        gone = u[::2]
        batch = np.concatenate([gone, np.array([1 << 63, (1 << 63) + 5], dtype=np.uint64), gone[:7], gone[:1]])
        batch = np.random.default_rng(42).permutation(batch)
        nk, npos = ix.erase(batch)
        assert nk == len(gone) and npos == int(m.count(gone).sum())
        assert twin.erase(batch) == len(gone)
        keep = ~np.isin(keys, gone)
        check_against_model(ix, keys[keep], pos[keep], extra_queries=gone[:40])
        check_layout_against_twin(ix, twin, "farm")
        assert ix.erase(np.array([1 << 63], dtype=np.uint64)) == (0, 0)       # misses only
        check_against_model(ix, keys[keep], pos[keep])
        assert ix.erase(np.zeros(0, dtype=np.uint64)) == (0, 0)
    finally:
        twin.close()


def test_erase_the_key_with_a_segment_of_two_tiles(ix):
    lens = [1] * 20 + [2 * T] + [3] * 20
    ks = distinct_keys(len(lens), 51)
    keys, pos = pairs_of(ks, lens, 52)
    ix.build(keys, pos)
    assert ix.erase(ks[20:21]) == (1, 2 * T)
    keep = keys != ks[20]
    check_against_model(ix, keys[keep], pos[keep], extra_queries=ks[20:21])


def test_erase_everything_then_append_again(ix):
    """erasing every key leaves a usable empty index on the table as kh_erase left it: it keeps its capacity (a cleared table, not the
    fresh one kh_index_clear gives), and what follows is laid out like the twin with the same history"""
    ks = distinct_keys(3000, 61)
    keys, pos = pairs_of(ks, [2] * 3000, 62)
    twin = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43)
    try:
        ix.build(keys, pos)
        twin.insert_reduce_plus(keys)
        cap = ix.capacity()
        assert cap > 128
        assert ix.erase(ks) == (3000, 6000)
        assert twin.erase(ks) == 3000
        assert (ix.size(), ix.total(), ix.capacity()) == (0, 0, cap) and twin.capacity() == cap
        ek, eo, ep = ix.export()
        assert len(ek) == 0 and eo.tolist() == [0] and len(ep) == 0
        assert ix.count(ks[:5]).tolist() == [0] * 5
        fo, fp = ix.find(ks[:5])
        assert fo.tolist() == [0] * 6 and len(fp) == 0
        assert ix.erase(ks[:5]) == (0, 0) and ix.erase_counts(0, 2 ** 32 - 1) == (0, 0)
        k2, p2 = pairs_of(ks[:50], [3] * 50, 63)
        ix.append(k2, p2)
        twin.insert_reduce_plus(k2)
        check_against_model(ix, k2, p2)
        check_layout_against_twin(ix, twin, "farm")
        assert ix.erase(ks[:50]) == (50, 150)
        ix.build(k2, p2)                                                     # build works on the emptied index too
        check_against_model(ix, k2, p2)
        ix.clear()
        assert ix.capacity() == 128
    finally:
        twin.close()


def test_erase_then_append_a_key_again_returns_only_the_new_positions(ix):
    keys, pos = skewed_pairs(91)
    ix.build(keys, pos)
    m = IndexModel(keys, pos)
    hot = m.keys[np.argmax(m.counts)]
    assert ix.erase(np.array([hot], dtype=np.uint64)) == (1, int(m.counts.max()))
    newp = np.array([5, 1, 3], dtype=np.uint32)
    ix.append(np.full(3, hot, dtype=np.uint64), newp)
    fo, fp = ix.find(np.array([hot], dtype=np.uint64))
    assert fo.tolist() == [0, 3] and fp.tolist() == [1, 3, 5]
    keep = keys != hot
    check_against_model(ix, np.concatenate([keys[keep], np.full(3, hot, dtype=np.uint64)]), np.concatenate([pos[keep], newp]))


LENS = [1] * 40 + [2, 3, T - 1, T, T + 1, 2 * T]


@pytest.fixture
def lens_index():
    ks = distinct_keys(len(LENS), 101)
    keys, pos = pairs_of(ks, LENS, 102)
    x = kh.KmerPositionIndex(k=21)
    x.build(keys, pos)
    yield x, ks, keys, pos
    x.close()


def survivors(ks, keys, pos, lo, hi):
    lens = np.array(LENS)
    gone = ks[(lens >= lo) & (lens <= hi)]
    keep = ~np.isin(keys, gone)
    return gone, keys[keep], pos[keep], int(lens[(lens >= lo) & (lens <= hi)].sum())


def test_erase_counts_a_range(lens_index):
    x, ks, keys, pos = lens_index
    twin = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43)
    try:
        twin.insert_reduce_plus(keys)
        gone, k2, p2, npos = survivors(ks, keys, pos, 2, 3)
        assert x.erase_counts(2, 3) == (2, 5) and npos == 5
        assert twin.erase(gone) == 2
        check_against_model(x, k2, p2, extra_queries=gone)
        check_layout_against_twin(x, twin, "farm")
    finally:
        twin.close()


def test_drop_above(lens_index):
    x, ks, keys, pos = lens_index
    gone, k2, p2, npos = survivors(ks, keys, pos, T, 2 ** 32 - 1)
    assert len(gone) == 3
    assert x.drop_above(T - 1) == (3, npos) and npos == 4 * T + 1
    check_against_model(x, k2, p2, extra_queries=gone)
    assert int(np.diff(x.export()[1].astype(np.int64)).max()) == T - 1
    assert x.drop_above(2 ** 32 - 1) == (0, 0)


def test_erase_counts_that_match_nothing_change_no_byte(lens_index):
    x, ks, keys, pos = lens_index
    before = x.export()
    assert x.erase_counts(4, T - 2) == (0, 0)
    assert x.erase_counts(2 * T + 1, 2 ** 32 - 1) == (0, 0)
    assert x.erase_counts(0, 0) == (0, 0)
    # lo > hi is the empty range, as in kh_erase_values: nothing is erased, the call succeeds
    assert x.erase_counts(3, 2) == (0, 0)
    assert x.erase_counts(2 ** 32 - 1, 0) == (0, 0)
    assert same_bytes(before, x.export())
    check_against_model(x, keys, pos)
    with pytest.raises(ValueError):
        x.erase_counts(-1, 5)
