"""GPU: the value-range operations -- value_histogram, count_values / select_values (host and device output) and erase_values -- on the
three tables (Robin Hood and linear probing with 64-bit keys, Robin Hood with 16-byte keys) under the identity and the murmur hash.

Every expectation comes from numpy applied to the table's OWN to_vector() (slot order), or, for erase_values, from a twin table built
identically that gets erase() of the keys numpy selects: the two must then agree in size, capacity, info array, to_vector() and
find_values over all original keys.  to_vector() of the twins is compared in slot order UP TO the order of elements that share one
home bucket: that order is decided by LDS atomics in the tables' re-layout kernels, and two tables built by the very same calls
already differ in it before anything is erased (measured on the MI355X: 100 keys, identity hash) -- see canon().  For the same reason
the info arrays of two LP twins agree after a tombstone erase in their clusters and tombstone counts, not slot by slot; the table's
own array is checked slot by slot instead.  Shapes: an empty table at capacity 128, 100 keys (one partial workgroup), 5 000 (more than one
2048-slot tile, ragged tail), 300 000 (several grid strides, more than 128 tiles) and one case of 1.2e6 keys.  Values hold 0, 1,
nbins-2, nbins-1, nbins, 2^31 and 2^32-1 (a signed comparison fails), one case holds a single value throughout (the wave-combining
path of the histogram), one real counts from insert_reduce_plus."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NBINS = 64
U32 = 0xFFFFFFFF
KINDS = ["rh", "lp", "wide"]
HASHES = ["identity", "murmur3avx64"]
SIZES = [0, 100, 5000, 300000]


def make(kind, hash, capacity=128):
    import kmerhash_amd as kh
    from kmerhash_amd.wide import hashmap_robinhood_doubling_wide
    cls = {"rh": kh.hashmap_robinhood_doubling, "lp": kh.hashmap_linearprobe_doubling, "wide": hashmap_robinhood_doubling_wide}[kind]
    return cls(capacity, hash=hash)


def make_keys(kind, n, seed=3):
    from kmerhash_amd import workloads as W
    k = W.distinct_u64(n, seed=seed)
    if kind != "wide":
        return k
    w = np.ascontiguousarray(np.stack([k, W.distinct_u64(n, seed=seed + 100)], axis=1))
    m = len(w[1::7])
    w[1::7, 0] = w[0::7, 0][:m]             # pairs that share w0 (one home bucket under the identity hash) and differ in w1
    return w


def make_vals(n, seed=5):
    """uniform in 0..99 plus the values on which a bin edge or a signed comparison goes wrong"""
    v = np.random.RandomState(seed).randint(0, 100, size=n).astype(np.uint32)
    special = np.array([0, 1, NBINS - 2, NBINS - 1, NBINS, 1 << 31, U32], dtype=np.uint64).astype(np.uint32)
    if n >= 3 * len(special):
        v[: 3 * len(special)] = np.tile(special, 3)
    return v


def build(kind, hash, n, vals=None, seed=3):
    t = make(kind, hash)
    keys = make_keys(kind, n, seed)
    vals = make_vals(n) if vals is None else vals
    if n:
        assert t.insert(keys, vals) == n
    return t, keys, vals


def np_hist(v, nbins):
    return np.bincount(np.minimum(v.astype(np.int64), nbins - 1), minlength=nbins).astype(np.uint64)


def in_range(v, lo, hi):
    return (v >= np.uint32(lo)) & (v <= np.uint32(hi)) if lo <= hi else np.zeros(len(v), dtype=bool)


def dev_np(keys, vals):
    return keys.cpu().numpy().view(np.uint64), vals.cpu().numpy().view(np.uint32)


def check_hist(t, nbins_list=(NBINS, 1, 16384)):
    _, v = t.to_vector()
    for nbins in nbins_list:
        h = t.value_histogram(nbins)
        assert h.dtype == np.uint64 and h.shape == (nbins,)
        assert np.array_equal(h, np_hist(v, nbins)), nbins
        assert int(h.sum()) == t.size()
    assert t.value_histogram(1).tolist() == [t.size()]


RANGES = [(0, U32), (1, NBINS - 2), (NBINS - 1, 1 << 31), (1 << 31, U32), (5, 5), (U32, U32), (0, 0), (9, 3), (U32, 0)]


def check_select(t, ranges=RANGES):
    k, v = t.to_vector()
    for lo, hi in ranges:
        m = in_range(v, lo, hi)
        assert t.count_values(lo, hi) == int(m.sum()), (lo, hi)
        hk, hv = t.select_values(lo, hi)
        assert hk.dtype == np.uint64 and hv.dtype == np.uint32 and hk.shape == k[m].shape
        assert np.array_equal(hk, k[m]) and np.array_equal(hv, v[m]), (lo, hi)            # equal AND in slot order
        dk, dv = t.select_values(lo, hi, device=True)
        assert dk.is_cuda and dv.is_cuda and tuple(dk.shape) == k[m].shape
        dk, dv = dev_np(dk, dv)
        assert np.array_equal(dk, k[m]) and np.array_equal(dv, v[m]), (lo, hi)
    fk, fv = t.select_values(0, U32)
    assert np.array_equal(fk, k) and np.array_equal(fv, v)                                # the full range is to_vector()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_histogram_and_select_match_numpy_on_to_vector(kind, hash, n):
    t, keys, vals = build(kind, hash, n)
    assert t.size() == n and (n or t.capacity() == 128)
    if n >= 100:
        assert set([0, 1, NBINS - 2, NBINS - 1, NBINS, 1 << 31, U32]) <= set(t.to_vector()[1].tolist())
    check_hist(t)
    check_select(t)
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_one_short_is_refused_with_the_count(kind):
    from kmerhash_amd import _capi as K
    t, _, _ = build(kind, "murmur3avx64", 5000)
    _, v = t.to_vector()
    m = int(in_range(v, 10, 40).sum())
    assert m > 100
    words = 2 if kind == "wide" else 1
    for device in (False, True):
        n = C.c_uint64()
        if device:
            import torch
            ok = torch.full((m * words,), -1, dtype=torch.int64, device="cuda")
            ov = torch.full((m,), -1, dtype=torch.int32, device="cuda")
            kp, vp, where = ok.data_ptr(), ov.data_ptr(), K.KH_MEM_DEVICE
        else:
            ok, ov = np.zeros(m * words, dtype=np.uint64), np.zeros(m, dtype=np.uint32)
            kp, vp, where = ok.ctypes.data, ov.ctypes.data, K.KH_MEM_HOST
        assert t._fn("select_values")(t._h, 10, 40, where, kp, vp, m - 1, C.byref(n)) == K.KH_ERR_INVALID
        assert n.value == m
        assert t._fn("select_values")(t._h, 10, 40, where, kp, vp, m, C.byref(n)) == K.KH_OK and n.value == m
        # keys only (out_vals NULL) and count only (out_keys NULL)
        assert t._fn("select_values")(t._h, 10, 40, where, kp, None, m, C.byref(n)) == K.KH_OK and n.value == m
        n.value = 0
        assert t._fn("select_values")(t._h, 10, 40, where, None, None, 0, C.byref(n)) == K.KH_OK and n.value == m
    t.close()


@pytest.mark.parametrize("kind", KINDS)
def test_bad_nbins_is_invalid(kind):
    import kmerhash_amd as kh
    from kmerhash_amd import _capi as K
    t, _, _ = build(kind, "murmur3avx64", 100)
    for nbins in (0, 16385):
        with pytest.raises(kh.KhError) as e:
            t.value_histogram(nbins)
        assert e.value.status == K.KH_ERR_INVALID
    assert t.value_histogram(16384).shape == (16384,)
    t.close()


@pytest.mark.parametrize("n", [100, 5000, 300000])
@pytest.mark.parametrize("value", [7, NBINS - 1, U32])
@pytest.mark.parametrize("kind", KINDS)
def test_every_value_equal(kind, value, n):
    """every lane of every wave holds the same bin: the wave-combining path of the histogram kernel"""
    t, _, _ = build(kind, "murmur3avx64", n, vals=np.full(n, value, dtype=np.uint32))
    check_hist(t)
    h = t.value_histogram(NBINS)
    assert int(h[min(value, NBINS - 1)]) == n
    assert t.count_values(value, value) == n and t.count_values(0, value - 1) == 0
    t.close()


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_real_counts_from_insert_reduce_plus(kind, hash):
    """a k-mer counter's table: nearly all counts 1 or 2, a few large"""
    base = make_keys(kind, 40000, seed=9)
    mult = np.ones(len(base), dtype=np.int64)
    mult[::3] = 2
    mult[::1000] = 300
    batch = np.repeat(base, mult, axis=0)
    batch = batch[np.random.RandomState(1).permutation(len(batch))]
    t = make(kind, hash)
    assert t.insert_reduce_plus(batch) == len(base)
    assert t.insert_reduce_plus(batch[:5000]) == 0
    k, v = t.to_vector()
    assert int(v.astype(np.int64).sum()) == len(batch) + 5000 and v.max() >= 300
    check_hist(t, (256, NBINS, 2))
    check_select(t, [(1, 1), (2, 2), (3, U32), (0, 0), (1, U32)])
    assert t.value_histogram(256)[0] == 0
    t.close()


@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_tables_that_have_been_erased_from(kind, hash):
    """LP tombstones are neither counted nor selected; a Robin Hood table after a batch erase carries no marks"""
    t, keys, vals = build(kind, hash, 5000)
    assert t.erase(keys[1000:2000]) == 1000                    # LP: 1000 tombstones (4000 of 16384 slots >= min load 3276: no shrink)
    if kind == "lp":
        assert t.capacity() == 16384 and int((t.export_info() == 0x80).sum()) == 1000
    assert t.size() == 4000
    check_hist(t)
    check_select(t)
    left = np.concatenate([vals[:1000], vals[2000:]])
    assert np.array_equal(t.value_histogram(NBINS), np_hist(left, NBINS))
    assert t.erase_values(0, 49) == int((left < 50).sum())
    check_hist(t)
    check_select(t)
    t.close()


def canon(t, kind, hash):
    """to_vector() in slot order with every run of elements that share a home bucket sorted by key: the slot order as far as the
    table defines it (a re-layout ranks the elements of one home bucket with an LDS atomic, so their mutual order differs between
    two tables built by the same calls).  An element that changes place with one of ANOTHER home bucket changes the result."""
    import kmerhash_amd as kh
    from kmerhash_amd.wide import hash_batch_wide
    k, v = t.to_vector()
    if len(v) == 0:
        return k, v
    h = (hash_batch_wide(k, hash=hash, seed=43) if kind == "wide" else kh.hash_batch(k, hash=hash, seed=43)) & np.uint64(t.capacity() - 1)
    # the table is circular: a home bucket's run may wrap from the last slots to slot 0, and which of its elements wrap is again
    # their mutual order.  Slot order is home order up to that rotation: start the sequence at the run of the smallest home bucket
    first = (h == h.min()) & (np.roll(h, 1) != h.min())
    if first.any():
        lead = int(np.argmax(first))
        k, v, h = np.roll(k, -lead, axis=0), np.roll(v, -lead), np.roll(h, -lead)
    run = np.concatenate([[0], np.cumsum(h[1:] != h[:-1])])
    order = np.lexsort((k[:, 1], k[:, 0], run)) if kind == "wide" else np.lexsort((k, run))
    return k[order], v[order]


def same_items(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


ERASE_RANGES = {"none": (100, (1 << 31) - 1), "tenth": (10, 19), "most": (0, 59), "all": (0, U32), "high": (1 << 31, U32)}


def twin_erase(kind, hash, n, lo, hi):
    a, keys, vals = build(kind, hash, n)
    b, _, _ = build(kind, hash, n)
    kb, vb = b.to_vector()
    assert a.capacity() == b.capacity() and np.array_equal(a.export_info(), b.export_info())
    assert same_items(canon(a, kind, hash), canon(b, kind, hash)), "the twins differ before anything was erased"
    sel = in_range(vb, lo, hi)
    want = int(sel.sum())
    cap0 = a.capacity()
    if kind == "lp":            # what a tombstone erase must leave in A's own info array
        info0, (_, sv) = a.export_info(), a.export_slots()
        expect = info0.copy()
        expect[(info0 < 0x40) & in_range(sv, lo, hi)] = 0x80
    assert a.erase_values(lo, hi) == want
    assert b.erase(kb[sel]) == want
    assert a.size() == b.size() == n - want
    assert a.capacity() == b.capacity()
    ia, ib = a.export_info(), b.export_info()
    if kind == "lp" and a.capacity() == cap0:
        # tombstones in place: WHICH slot of a home bucket's run holds the erased key differs between the twins like the order in
        # canon(); the clusters and the number of tombstones agree, and A's array is exactly its old one with the matches marked
        assert np.array_equal(ia != 0x40, ib != 0x40) and int((ia == 0x80).sum()) == int((ib == 0x80).sum()) == want
        assert np.array_equal(ia, expect)
    else:
        assert np.array_equal(ia, ib)
    assert same_items(canon(a, kind, hash), canon(b, kind, hash))
    fa, fb = a.find_values(keys), b.find_values(keys)
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    assert int(np.asarray(fa[1]).sum()) == n - want
    assert np.array_equal(np.asarray(fa[1]).astype(bool), ~in_range(vals, lo, hi))
    assert a.erase_values(lo, hi) == 0 and a.size() == n - want                         # a second call erases nothing
    assert a.count_values(lo, hi) == 0
    # the table accepts inserts afterwards
    fresh = make_keys(kind, 300, seed=77)
    assert a.insert(fresh, np.full(300, 12, dtype=np.uint32)) == 300
    assert a.size() == n - want + 300
    fv, ff = a.find_values(fresh)
    assert np.asarray(ff).all() and (np.asarray(fv) == 12).all()
    check_hist(a, (NBINS,))
    return cap0, a, b


@pytest.mark.parametrize("which", sorted(ERASE_RANGES))
@pytest.mark.parametrize("n", [100, 5000, 300000])
@pytest.mark.parametrize("hash", HASHES)
@pytest.mark.parametrize("kind", KINDS)
def test_erase_values_equals_erase_of_the_selected_keys(kind, hash, n, which):
    lo, hi = ERASE_RANGES[which]
    cap0, a, b = twin_erase(kind, hash, n, lo, hi)
    a.close()
    b.close()


@pytest.mark.parametrize("hash", HASHES)
def test_lp_erase_values_crosses_the_shrink_threshold(hash):
    """5000 keys at capacity 16384; erasing ~60 % leaves fewer than min_load = 0.2 x 16384: the LP table shrinks as after erase()"""
    a, keys, vals = build("lp", hash, 5000)
    b, _, _ = build("lp", hash, 5000)
    assert a.capacity() == 16384
    kb, vb = b.to_vector()
    sel = in_range(vb, 0, 59)
    assert 5000 - int(sel.sum()) < int(np.float32(16384) * np.float32(0.2))
    assert a.erase_values(0, 59) == b.erase(kb[sel]) == int(sel.sum())
    assert a.capacity() == b.capacity() < 16384
    assert np.array_equal(a.export_info(), b.export_info()) and not (a.export_info() == 0x80).any()
    assert same_items(canon(a, "lp", hash), canon(b, "lp", hash))
    # Robin Hood never shrinks on a batch erase
    r, _, _ = build("rh", hash, 5000)
    cap = r.capacity()
    assert r.erase_values(0, 98) > 4000 and r.capacity() == cap
    a.close(); b.close(); r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_one_large_table(kind):
    n = 1_200_000
    t, keys, vals = build(kind, "murmur3avx64", n)
    check_hist(t, (NBINS, 256))
    check_select(t, [(0, U32), (10, 10), (1 << 31, U32)])
    t.close()
    cap0, a, b = twin_erase(kind, "murmur3avx64", n, 10, 19)
    a.close()
    b.close()


def _guarded(t, K, kh):
    for call in (lambda: t.value_histogram(NBINS), lambda: t.count_values(0, U32), lambda: t.select_values(0, 5),
                 lambda: t.select_values(0, U32, device=True), lambda: t.erase_values(0, U32)):
        with pytest.raises(kh.KhError) as e:
            call()
        assert e.value.status == K.KH_ERR_INVALID


@pytest.mark.parametrize("kind", ["rh", "wide_stream"])
def test_refused_during_a_streamed_insert(kind):
    import kmerhash_amd as kh
    from kmerhash_amd import _capi as K
    from kmerhash_amd.wide import hashmap_robinhood_doubling_wide_stream
    wide = kind == "wide_stream"
    t = hashmap_robinhood_doubling_wide_stream(128, hash="murmur3avx64") if wide else kh.hashmap_robinhood_doubling(128, hash="murmur3avx64")
    keys = make_keys("wide" if wide else "rh", 5000)
    vals = make_vals(5000)
    assert t.insert(keys[:1000], vals[:1000]) == 1000
    t.insert_begin(4000)
    _guarded(t, K, kh)
    t.insert_feed(keys[1000:3000], vals[1000:3000])
    _guarded(t, K, kh)
    t.insert_feed(keys[3000:], vals[3000:])
    assert t.insert_end() == 4000                                 # the streamed insert still completes
    assert t.size() == 5000
    check_hist(t, (NBINS,))
    check_select(t, [(0, U32), (10, 19)])
    assert t.erase_values(10, 19) == int(in_range(vals, 10, 19).sum())
    t.close()
