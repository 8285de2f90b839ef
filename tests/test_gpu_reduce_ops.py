"""Reducer inserts beyond std::plus: min, max and bit-or (kh_insert_reduce / kh_wide_insert_reduce and their streamed flags).

The check is the same everywhere.  A TWIN table receives the same keys through insert_reduce_plus in the same calls: the table under
test must equal it in size(), capacity() and export_info() -- the reference runs one code path for every Reducer, so only the values
may differ -- and its sorted_items() must hold the twin's keys with the values of a numpy group-reduce (ufunc.reduceat over the
key-sorted batch) combined with the values held before.  Values are drawn over the whole 32-bit range, 0 and 0xFFFFFFFF included;
half of them are thinned out (the AND of three draws) so that a bit-or over forty occurrences does not saturate.

Every comparison is between integers: bit-exact, no tolerance.  The two constructions taken from test_gpu_parity.py (class restart,
repeatable streamed insert with hidden skew) run with the one operation the issue names for them; everything else runs for all three.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402

OPS = ["min", "max", "or"]
UFUNC = {"plus": np.add, "min": np.minimum, "max": np.maximum, "or": np.bitwise_or}
RH, LP, WIDE = kh.hashmap_robinhood_doubling, kh.hashmap_linearprobe_doubling, kh.hashmap_robinhood_doubling_wide
NARROW = [("rh", RH), ("lp", LP)]
ALL = NARROW + [("wide", WIDE)]


def dev(a):
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def draw_vals(n, seed):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 1 << 32, (3, n), dtype=np.uint64).astype(np.uint32)
    v = np.where(rng.integers(0, 2, n) == 1, r[0], r[0] & r[1] & r[2])
    v[rng.integers(0, n, max(2, n // 16))] = 0
    v[rng.integers(0, n, max(2, n // 16))] = 0xFFFFFFFF
    v[0] = 0
    v[n - 1] = 0xFFFFFFFF
    return v.astype(np.uint32)


def make_keys(cls, n, seed):
    """n distinct keys of the table's width"""
    k = W.distinct_u64(n, seed=seed)
    if cls is WIDE or (isinstance(cls, type) and issubclass(cls, WIDE)):
        return np.stack([k, W.distinct_u64(n, seed=seed + 1000) >> np.uint64(40)], axis=1)       # (w0, w1)
    return k


def order_of(keys):
    """the order of sorted_items(): by key, wide keys by (w1, w0)"""
    return np.argsort(keys, kind="stable") if keys.ndim == 1 else np.lexsort((keys[:, 0], keys[:, 1]))


def group_reduce(keys, vals, op):
    """-> (distinct keys in sorted_items() order, op over the values of each key's occurrences)"""
    o = order_of(keys)
    ks, vs = keys[o], vals[o]
    diff = ks[1:] != ks[:-1]
    starts = np.flatnonzero(np.r_[True, diff if ks.ndim == 1 else diff.any(axis=1)])
    return ks[starts], UFUNC[op].reduceat(vs, starts).astype(np.uint32)


def combined(before, bk, bv, op):
    """the items a table that held `before` = (keys, vals) holds after a reduce-insert of the batch (bk, bv)"""
    rk, rv = group_reduce(bk, bv, op)
    return group_reduce(np.concatenate([before[0], rk]), np.concatenate([before[1], rv]), op)


def same_structure(g, twin):
    assert g.size() == twin.size()
    assert g.capacity() == twin.capacity()
    assert np.array_equal(g.export_info(), twin.export_info())


def check(g, twin, exp):
    same_structure(g, twin)
    gk, gv = g.sorted_items()
    tk, _ = twin.sorted_items()
    assert np.array_equal(gk, tk)
    assert np.array_equal(gk, exp[0])
    assert np.array_equal(gv, exp[1])


def pair(cls, cap=128, **kw):
    return cls(cap, 0.35, 0.8, **kw), cls(cap, 0.35, 0.8, **kw)


def preload(g, twin, keys, vals):
    assert g.insert(dev(keys), dev(vals)) == twin.insert(dev(keys), dev(vals)) == len(keys)
    return g.sorted_items()


def dup_batch(present, new, n, seed):
    """n records over the given present and new keys, every key at least once, shuffled"""
    pool = np.concatenate([present, new])
    rng = np.random.default_rng(seed)
    idx = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n - len(pool))])
    return pool[rng.permutation(idx)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kname,cls", NARROW)
def test_small_batch_kernel(kname, cls, op):
    """12 records, 5 distinct keys of which 2 are in a table of 1000 keys: k_small_batch applies reduc(stored, incoming) one by one"""
    g, twin = pair(cls)
    base = make_keys(cls, 1000, 11)
    before = preload(g, twin, base, draw_vals(1000, 12))
    new = make_keys(cls, 3, 13)
    bk = dup_batch(base[[3, 500]], new, 12, 14)
    bv = draw_vals(12, 15)
    g.profile_enable(True)
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == 3
    p = g.profile()
    assert "k_small_batch" in p and "k_dedup" not in p, p
    check(g, twin, combined(before, bk, bv, op))
    g.close(); twin.close()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kname,cls", ALL)
def test_general_path_empty_table_heavy_duplicates(kname, cls, op):
    """60 000 records over 1 500 distinct keys into an empty table of capacity 128.  The partitions are cut for the capacity that 60 000
    DISTINCT keys would need (64 of them, about 940 records each: one round of the 2048-record staging area), so three of the keys take
    6 000 records each: whatever the partitioning, their partitions hold more than 6 000 records and stream through the staging area
    in several rounds, the representatives compacted to the front in between.  The values of those three keys are made so that every
    round counts: for min / max they are distinct draws (one smallest, one largest record, anywhere in the stream), for or sixteen bits
    are each carried by ONE record.  Everything else draws over the whole 32-bit range."""
    g, twin = pair(cls)
    new = make_keys(cls, 1500, 21)
    rng = np.random.default_rng(24)
    bk = np.concatenate([dup_batch(new[:0], new, 42_000, 22), np.repeat(new[[7, 700, 1400]], 6000, axis=0)])
    bv = draw_vals(60_000, 23)
    if op == "or":
        r = rng.integers(0, 1 << 32, (3, 18_000), dtype=np.uint64).astype(np.uint32)
        hot = r[0] & r[1] & r[2] & np.uint32(0xFFF)
        for j in range(3):
            at = 6000 * j + rng.choice(6000, 16, replace=False)
            hot[at] |= np.uint32(1) << np.arange(14, 30, dtype=np.uint32)
    else:
        hot = rng.choice(np.arange(0x1000, 0x7FFF0000, 0x1001, dtype=np.uint32), 18_000, replace=False)
    bv[42_000:] = hot
    mix = rng.permutation(60_000)
    bk, bv = bk[mix], bv[mix]
    assert len(group_reduce(bk, bv, op)[0]) == 1500
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == 1500
    check(g, twin, group_reduce(bk, bv, op))
    # host memory takes the same way
    g2, _ = pair(cls)
    assert g2.insert_reduce(bk, bv, op) == 1500
    check(g2, twin, group_reduce(bk, bv, op))
    g.close(); g2.close(); twin.close()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kname,cls", ALL)
def test_general_path_loaded_table_doubling(kname, cls, op):
    """a table of 30 000 keys, 200 000 records over 60 000 distinct keys, half of them present: the apply kernel for the keys the table
    holds, new keys, and the capacity grows"""
    g, twin = pair(cls)
    keys = make_keys(cls, 60_000, 31)
    before = preload(g, twin, keys[:30_000], draw_vals(30_000, 32))
    cap0 = g.capacity()
    bk = dup_batch(keys[:30_000], keys[30_000:], 200_000, 33)
    bv = draw_vals(200_000, 34)
    if cls is not WIDE:
        g.profile_enable(True)
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == 30_000
    if cls is not WIDE:
        p = g.profile()
        assert "k_dedup" in p and "k_apply_reduce" in p and "k_insert_fused" not in p and "k_apply_plus" not in p, p
    assert g.capacity() > cap0
    check(g, twin, combined(before, bk, bv, op))
    g.close(); twin.close()


@pytest.mark.parametrize("op", OPS)
def test_in_place_path(op):
    """Robin Hood at capacity 2^20 with 5e5 keys, 1 500 records (half of the keys present, duplicates): applied in place, no re-layout"""
    g, twin = pair(RH, 1 << 20)
    keys = make_keys(RH, 500_400, 41)
    before = preload(g, twin, keys[:500_000], draw_vals(500_000, 42))
    bk = dup_batch(keys[1000:1400], keys[500_000:], 1500, 43)
    bv = draw_vals(1500, 44)
    g.profile_enable(True)
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == 400
    p = g.profile()
    assert "k_ip_apply" in p and "k_apply_reduce" in p, p
    assert "k_chunk_place" not in p and "k_rebuild_fused" not in p and "k_insert_fused" not in p, p
    assert g.capacity() == 1 << 20
    check(g, twin, combined(before, bk, bv, op))
    g.close(); twin.close()


@pytest.mark.parametrize("op", OPS)
def test_linear_probe_with_tombstones(op):
    """erase 10 000 of 30 000 keys, then a batch that names erased, present and new keys"""
    g, twin = pair(LP)
    keys = make_keys(LP, 35_000, 51)
    vals = draw_vals(30_000, 52)
    preload(g, twin, keys[:30_000], vals)
    assert g.erase(dev(keys[:10_000])) == twin.erase(dev(keys[:10_000])) == 10_000
    before = g.sorted_items()
    assert len(before[0]) == 20_000
    same_structure(g, twin)
    bk = dup_batch(np.concatenate([keys[5_000:10_000], keys[10_000:15_000]]), keys[30_000:], 40_000, 53)
    bv = draw_vals(40_000, 54)
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == 10_000
    check(g, twin, combined(before, bk, bv, op))
    # a handful more into the tombstoned table: the small-batch kernel reuses deleted slots.  WHICH slot an element of a linear-probe
    # table sits in depends on the route that laid the table out (the twin's std::plus batch above may take a one-launch form), so the
    # tombstones of this second erase need not lie in the same slots: sizes, occupied-slot counts and items are compared
    assert g.erase(dev(keys[20_000:22_000])) == twin.erase(dev(keys[20_000:22_000])) == 2000
    before = g.sorted_items()
    bk = dup_batch(keys[[20_000, 25_000, 26_000]], make_keys(LP, 2, 55), 10, 56)
    bv = draw_vals(10, 57)
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == 3
    assert g.size() == twin.size() and g.capacity() == twin.capacity()
    assert int((g.export_info() < 0x40).sum()) == int((twin.export_info() < 0x40).sum()) == g.size()
    exp = combined(before, bk, bv, op)
    gk, gv = g.sorted_items()
    assert np.array_equal(gk, twin.sorted_items()[0]) and np.array_equal(gk, exp[0]) and np.array_equal(gv, exp[1])
    g.close(); twin.close()


def _fmix64(k):
    k = k.astype(np.uint64).copy()
    k ^= k >> np.uint64(33); k *= np.uint64(0xff51afd7ed558ccd); k ^= k >> np.uint64(33); k *= np.uint64(0xc4ceb9fe1a85ec53); k ^= k >> np.uint64(33)
    return k


def test_class_restart_applies_once():
    """the construction of test_reducer_plus_class_restart_counts_once with max: 3400 keys of one partition of an in-place batch, 900 in
    class 0 of R = 2 (fits) and 2500 in class 1 (overflows -> R = 4, everything again).  All keys exist already.  A sweep that is
    abandoned must not have touched the table -- with max the damage could not be undone -- and the list it wrote must be forgotten."""
    n0 = 2_000_000
    uni = W.distinct_u64(n0, seed=31)
    g, twin = pair(RH)
    before = preload(g, twin, uni, draw_vals(n0, 61))
    assert g.capacity() == 1 << 22
    h = kh.hash_batch(uni[:400_000], "murmur3avx64", 43)
    part0 = ((h >> np.uint64(11)) & np.uint64(3)) == 0
    cls1 = ((_fmix64(uni[:400_000] + np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)) % np.uint64(2)) == 1
    c0 = uni[:400_000][part0 & ~cls1][:900]
    c1 = uni[:400_000][part0 & cls1][:2500]
    assert len(c0) == 900 and len(c1) == 2500
    bk = np.concatenate([c0, c1, c0[:300]])
    bk = bk[W.shuffle_perm(len(bk), 1)]
    bv = draw_vals(len(bk), 62)
    g.profile_enable(True)
    assert g.insert_reduce(dev(bk), dev(bv), "max") == twin.insert_reduce_plus(dev(bk)) == 0
    p = g.profile()
    assert "k_part_direct" in p and "k_apply_reduce" in p, p
    check(g, twin, combined(before, bk, bv, "max"))
    g.close(); twin.close()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kname,cls", NARROW + [("wide", kh.hashmap_robinhood_doubling_wide_stream)])
def test_streamed_form(kname, cls, op):
    """three feeds of unequal size equal the one-call form; insert_abort leaves items, capacity and info bytes as they were"""
    g, twin = pair(cls)
    keys = make_keys(cls, 30_000, 71)
    before = preload(g, twin, keys[:10_000], draw_vals(10_000, 72))
    bk = dup_batch(keys[:10_000], keys[10_000:], 90_000, 73)
    bv = draw_vals(90_000, 74)
    cuts = [0, 50_001, 50_018, 90_000]
    g.insert_begin(90_000, reduce=op)
    twin.insert_begin(90_000, reduce_plus=True)
    for a, b in zip(cuts[:-1], cuts[1:]):
        g.insert_feed(dev(bk[a:b]), dev(bv[a:b]))
        twin.insert_feed(dev(bk[a:b]))
    assert g.insert_end() == twin.insert_end() == 20_000
    exp = combined(before, bk, bv, op)
    check(g, twin, exp)
    one, _ = pair(cls)
    one.insert(dev(keys[:10_000]), dev(draw_vals(10_000, 72)))
    one.insert_reduce(dev(bk), dev(bv), op)
    check(one, g, exp)
    # abort
    info = g.export_info().copy()
    g.insert_begin(5000, reduce=op, repeatable=True)
    g.insert_feed(dev(bk[:3000]), dev(bv[:3000]))
    g.insert_abort()
    assert np.array_equal(g.export_info(), info)
    check(g, twin, exp)
    # a feed without values is refused for these operations; the streamed insert can still be given up
    g.insert_begin(10, reduce=op)
    with pytest.raises(kh.KhError):
        g.insert_feed(dev(bk[:10]))
    g.insert_abort()
    check(g, twin, exp)
    g.close(); twin.close(); one.close()


@pytest.mark.parametrize("kname,cls", NARROW)
def test_repeatable_streamed_with_hidden_skew(kname, cls):
    """the construction of test_reducer_plus_speculation_never_touches_live_counts with min: one key 30 000 times among 4e6 records
    at positions the sample does not look at overflows a slot of the histogram-free partition.  KhRetry must leave the table unchanged
    in items, capacity and info bytes -- a min that had been applied before the overflow flag was read could not be taken back -- and
    the plain re-feed gives numpy's result."""
    n = 4_000_000
    base = W.distinct_u64(1000, seed=3)
    fresh = W.distinct_u64(n, seed=4)
    k = fresh.copy()
    cand = np.arange(n)
    cand = cand[(cand % 61 != 0) & (cand % 22 != 0)]
    k[cand[::100][:30_000]] = fresh[7]
    k[(n // 65536) * np.arange(40_000, 40_600) + 2] = base[:600]
    k[(n // 65536) * np.arange(41_000, 41_100) + 2] = base[:100]
    v = draw_vals(n, 81)
    g, twin = pair(cls)
    pre = preload(g, twin, base, draw_vals(1000, 82))
    before = g.sorted_items(), g.capacity(), g.export_info().copy()
    cuts = [0, 1_500_000, 2_500_000, n]
    dk, dv = dev(k), dev(v)

    def feed_all(t, vals, **kw):
        t.insert_begin(n, **kw)
        for a, b in zip(cuts[:-1], cuts[1:]):
            t.insert_feed(dk[a:b], vals[a:b] if vals is not None else None)
        return t.insert_end()

    with pytest.raises(kh.KhRetry):
        feed_all(g, dv, reduce="min", repeatable=True)
    after = g.sorted_items(), g.capacity(), g.export_info()
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and before[1] == after[1]
    assert np.array_equal(before[2], after[2])
    assert feed_all(g, dv, reduce="min") == feed_all(twin, None, reduce_plus=True)
    check(g, twin, combined(pre, k, v, "min"))
    g.close(); twin.close()


def _revcomp(x, k):
    """reverse complement of 2-bit packed k-mers (first base most significant, A0 C1 G2 T3)"""
    out = np.zeros_like(x)
    for i in range(k):
        out |= (np.uint64(3) - ((x >> np.uint64(2 * i)) & np.uint64(3))) << np.uint64(2 * (k - 1 - i))
    return out


@pytest.mark.parametrize("op", OPS)
def test_key_transform(op):
    """a k-mer and its reverse complement are one key: both strands of a k-mer fold into one value.  Which strand's bits a NEW key
    stores is whichever occurrence claimed the fold's set entry (as for std::plus): keys are compared in canonical form."""
    K = 21
    g, twin = pair(RH)
    g.set_key_transform(K); twin.set_key_transform(K)
    fwd = W.distinct_u64(3000, seed=91) >> np.uint64(64 - 2 * K)
    canon = np.unique(np.minimum(fwd, _revcomp(fwd, K)))
    canon = canon[canon != _revcomp(canon, K)]
    rc = _revcomp(canon, K)
    m = len(canon)
    assert m > 2900
    half = m // 2
    pre_k = np.where(np.arange(half) % 2 == 0, canon[:half], rc[:half])      # the table holds either strand
    pre_v = draw_vals(half, 92)
    assert g.insert(dev(pre_k), dev(pre_v)) == twin.insert(dev(pre_k), dev(pre_v)) == half
    bk = dup_batch(canon, rc, 20_000, 93)                                      # every k-mer by both strands
    bv = draw_vals(20_000, 94)
    assert g.insert_reduce(dev(bk), dev(bv), op) == twin.insert_reduce_plus(dev(bk)) == m - half
    same_structure(g, twin)
    gk, gv = g.to_vector()
    gc = np.minimum(gk, _revcomp(gk, K))
    o = np.argsort(gc, kind="stable")
    ek, ev = combined((canon[:half], pre_v), np.minimum(bk, _revcomp(bk, K)), bv, op)
    assert np.array_equal(gc[o], ek) and np.array_equal(gv[o], ev)
    stored = dict(zip(gc.tolist(), gk.tolist()))
    assert all(stored[c] == s for c, s in zip(canon[:half].tolist(), pre_k.tolist()))      # keys held before keep their bits
    g.close(); twin.close()


@pytest.mark.parametrize("op", ["plus", "max"])
@pytest.mark.parametrize("kname,src_cls,dst_cls", [("rh_into_lp", RH, LP), ("wide_into_wide", WIDE, WIDE)])
def test_merge(kname, src_cls, dst_cls, op):
    """two tables of 50 000 keys with 20 000 in common: merge equals the numpy merge, `other` is unchanged"""
    keys = make_keys(src_cls, 80_000, 101)
    a, twin = pair(dst_cls)
    b = src_cls(128, 0.35, 0.8)
    ka, kb = keys[:50_000], keys[30_000:]
    va, vb = draw_vals(50_000, 102), draw_vals(50_000, 103)
    before = preload(a, twin, ka, va)
    assert b.insert(dev(kb), dev(vb)) == 50_000
    other = b.sorted_items(), b.capacity(), b.export_info().copy()
    assert a.merge(b, op=op) == twin.insert_reduce_plus(dev(kb)) == 30_000
    check(a, twin, combined(before, kb, vb, op))
    now = b.sorted_items(), b.capacity(), b.export_info()
    assert np.array_equal(other[0][0], now[0][0]) and np.array_equal(other[0][1], now[0][1]) and other[1] == now[1]
    assert np.array_equal(other[2], now[2])
    empty = src_cls(128, 0.35, 0.8)
    assert a.merge(empty, op=op) == 0
    check(a, twin, combined(before, kb, vb, op))
    a.close(); b.close(); twin.close(); empty.close()


def test_merge_refuses_another_key_width():
    n, w = RH(128, 0.35, 0.8), WIDE(128, 0.35, 0.8)
    with pytest.raises(ValueError):
        n.merge(w)
    with pytest.raises(ValueError):
        w.merge(n, op="max")
    with pytest.raises(ValueError):
        n.merge(n, op="xor")
    n.close(); w.close()


@pytest.mark.parametrize("kname,cls", ALL)
def test_plus_through_the_new_entry_point(kname, cls):
    """op="plus" is insert_reduce_plus, vals=None (every occurrence counts 1) included"""
    g, twin = pair(cls)
    keys = make_keys(cls, 3000, 111)
    bk = dup_batch(keys[:0], keys, 20_000, 112)
    bv = draw_vals(20_000, 113)
    assert g.insert_reduce(dev(bk), None, "plus") == twin.insert_reduce_plus(dev(bk)) == 3000
    assert g.insert_reduce(dev(bk), dev(bv), "plus") == twin.insert_reduce_plus(dev(bk), dev(bv)) == 0
    assert g.insert_reduce(bk[:10]) == twin.insert_reduce_plus(bk[:10]) == 0
    same_structure(g, twin)
    (gk, gv), (tk, tv) = g.sorted_items(), twin.sorted_items()
    assert np.array_equal(gk, tk) and np.array_equal(gv, tv)
    g.close(); twin.close()


@pytest.mark.parametrize("kname,cls", ALL)
def test_bad_arguments(kname, cls):
    import ctypes as C
    from kmerhash_amd import _capi as K
    g = cls(128, 0.35, 0.8)
    keys = make_keys(cls, 100, 121)
    vals = draw_vals(100, 122)
    with pytest.raises(ValueError):
        g.insert_reduce(dev(keys), None, "max")
    with pytest.raises(ValueError):
        g.insert_reduce(dev(keys), dev(vals), "xor")
    # the C entry points refuse the same: no values for max, an operation outside the enum
    fn = getattr(K.lib(), g.PREFIX + "insert_reduce")
    kk = np.ascontiguousarray(keys)
    out = C.c_uint64()
    assert fn(g._h, kk.ctypes.data, None, 100, K.KH_MEM_HOST, K.KH_REDUCE_MAX, C.byref(out)) == K.KH_ERR_INVALID
    assert fn(g._h, kk.ctypes.data, vals.ctypes.data, 100, K.KH_MEM_HOST, 4, C.byref(out)) == K.KH_ERR_INVALID
    begin = getattr(K.lib(), g.PREFIX + "insert_begin_ex")
    assert begin(g._h, 10, 2 << K.KH_INS_REDUCE_OP_SHIFT) == K.KH_ERR_INVALID      # an operation without KH_INS_REDUCE_PLUS
    assert begin(g._h, 10, 16) == K.KH_ERR_INVALID
    assert g.size() == 0
    assert g.insert_reduce(dev(keys), dev(vals), "or") == 100
    g.close()
