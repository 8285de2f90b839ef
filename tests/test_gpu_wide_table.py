"""GPU: the 16-byte-key Robin Hood table (kh_wide_*).  Equivalence with the 64-bit table under the identity hash, full-key equality,
the canonical Robin Hood layout under the real hashes (numpy (max,+) model over the homes), heavy duplication, probe overflow, scale."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from oracle.wide_model import rh_info_model  # noqa: E402      (the numpy (max,+) model over the homes: part of the wide-table CPU model)

M64 = (1 << 64) - 1
HASHES = ("murmur3avx64", "murmur", "farm")


def wide(w0, w1=None):
    w0 = np.asarray(w0, dtype=np.uint64)
    w1 = np.zeros_like(w0) if w1 is None else np.asarray(w1, dtype=np.uint64)
    return np.ascontiguousarray(np.stack([w0, w1], axis=1))


def assert_same(g, w, q):
    assert (g.size(), g.capacity()) == (w.size(), w.capacity())
    assert np.array_equal(g.export_info(), w.export_info())
    assert np.array_equal(g.displacement_histogram(), w.displacement_histogram())
    qw = wide(q)
    assert np.array_equal(g.count(q), w.count(qw))
    gv, gf = g.find_values(q)
    wv, wf = w.find_values(qw)
    assert np.array_equal(gf, wf) and np.array_equal(gv[gf == 1], wv[wf == 1])
    gk, gvv = g.find(q)
    wk, wvv = w.find(qw)
    assert np.array_equal(gk, wk[:, 0]) and not wk[:, 1].any() and np.array_equal(gvv, wvv)
    k64, v64 = g.sorted_items()
    kw, vw = w.sorted_items()
    assert np.array_equal(k64, kw[:, 0]) and np.array_equal(v64, vw)


def test_identity_hash_equivalence_with_64bit_table():
    """identity hash, w1 = 0: the wide table and the 64-bit table fed the same sequence agree call by call"""
    rng = np.random.default_rng(1)
    pool = rng.integers(0, 1 << 63, 300_000, dtype=np.uint64)
    g = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="identity")
    w = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash="identity")
    sizes = [0, 1, 5, 17, 300, 2048, 10_000, 65_536, 100_000]
    for step, n in enumerate(sizes + sizes[::-1]):
        keys = pool[rng.integers(0, len(pool), n)]            # duplicates included
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        op = step % 4
        if op == 0:
            assert g.insert(keys, vals) == w.insert(wide(keys), vals)
        elif op == 1:
            assert g.insert_reduce_plus(keys, vals) == w.insert_reduce_plus(wide(keys), vals)
        elif op == 2:
            assert g.insert_reduce_plus(keys) == w.insert_reduce_plus(wide(keys))
        else:
            assert g.erase(keys[: n // 2]) == w.erase(wide(keys[: n // 2]))
        q = np.concatenate([keys[: n // 3], pool[rng.integers(0, len(pool), 1000)]])
        assert_same(g, w, q)
        if step == 6:
            g.reserve(400_000); w.reserve(400_000)
            assert_same(g, w, q)
        if step == 12:
            g.rehash(1 << 12); w.rehash(1 << 12)
            assert_same(g, w, q)
    # device tensors: same results
    keys = pool[:50_000]
    dk = torch.from_numpy(wide(keys).view(np.int64)).cuda()
    vals = torch.arange(50_000, dtype=torch.int32, device="cuda")
    assert w.insert(dk, vals) == g.insert(torch.from_numpy(keys.view(np.int64)).cuda(), vals)
    assert np.array_equal(w.count(dk).cpu().numpy(), g.count(keys))
    fk, fv = w.find(dk)
    ok, ov = g.find(keys)
    assert np.array_equal(fk.cpu().numpy().view(np.uint64)[:, 0], ok) and np.array_equal(fv.cpu().numpy().view(np.uint32), ov)
    g.close(); w.close()


def test_full_key_equality():
    """keys sharing w0 but not w1: same home under the identity hash, distinct keys"""
    w = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash="identity")
    w0 = np.repeat(np.arange(1000, dtype=np.uint64) * 7919, 4)
    w1 = np.tile(np.array([0, 1, 1 << 63, M64], dtype=np.uint64), 1000)
    keys = wide(w0, w1)
    vals = np.arange(4000, dtype=np.uint32)
    assert w.insert(keys, vals) == 4000
    assert w.size() == 4000
    v, f = w.find_values(keys)
    assert f.all() and np.array_equal(v, vals)
    absent = wide(w0[::4], np.full(1000, 2, dtype=np.uint64))
    assert not w.count(absent).any()
    assert w.erase(keys[1::4]) == 1000
    c = w.count(keys)
    assert np.array_equal(c, np.tile(np.array([1, 0, 1, 1], dtype=np.uint8), 1000))
    w.close()


def expected_after(seq_ops):
    """dict model: first value wins / sums wrap mod 2^32"""
    d = {}
    for op, keys, vals in seq_ops:
        for k, v in zip(map(tuple, keys.tolist()), vals.tolist()):
            if op == "insert":
                d.setdefault(k, v)
            else:
                d[k] = (d.get(k, 0) + v) & 0xFFFFFFFF
    return d


@pytest.mark.parametrize("hname", HASHES)
def test_canonical_layout_under_real_hashes(hname):
    rng = np.random.default_rng(HASHES.index(hname) + 21)
    pool = wide(rng.integers(0, 1 << 64, 60_000, dtype=np.uint64, endpoint=False), rng.integers(0, 1 << 64, 60_000, dtype=np.uint64, endpoint=False))
    w = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash=hname, seed=43)
    g = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)          # bijective image (distinct w0s) for the capacities
    ops = []
    for step, n in enumerate([10, 1000, 20_000, 50_000, 3]):
        sel = rng.integers(0, len(pool), n)
        keys = pool[sel]
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if step % 2 == 0:
            w.insert(keys, vals); g.insert(sel.astype(np.uint64) + 1, vals); ops.append(("insert", keys, vals))
        else:
            w.insert_reduce_plus(keys, vals); g.insert_reduce_plus(sel.astype(np.uint64) + 1, vals); ops.append(("plus", keys, vals))
        d = expected_after(ops)
        assert w.size() == len(d) == g.size()
        assert w.capacity() == g.capacity()
        cap = w.capacity()
        allk = np.array(list(d.keys()), dtype=np.uint64).reshape(-1, 2)
        homes = kh.hash_batch_wide(allk, hname, 43) & np.uint64(cap - 1)
        assert np.array_equal(w.export_info(), rh_info_model(homes, cap))
        v, f = w.find_values(allk)
        assert f.all() and np.array_equal(v, np.array(list(d.values()), dtype=np.uint32))
    # the GPU hash equals the CPU statement (pinned by tests/test_wide_hash.py) on the first keys
    from oracle import oracle_py as O
    hb = kh.hash_batch_wide(pool[:64], hname, 43)
    for (a, b), h in zip(pool[:64].tolist(), hb.tolist()):
        data = int(a).to_bytes(8, "little") + int(b).to_bytes(8, "little")
        if hname == "murmur3avx64":
            x = O.murmur3_x86_128(data, 43); assert h == int(x[0]) | (int(x[1]) << 32)
        elif hname == "murmur":
            assert h == int(O.murmur3_x64_128(data, 43)[0])
    w.close(); g.close()


def test_heavy_duplication():
    w = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8)
    one = torch.tensor([[12345, -7]], dtype=torch.int64, device="cuda").repeat(1_000_000, 1)
    assert w.insert_reduce_plus(one) == 1
    v, f = w.find_values(one[:1])
    assert int(f[0]) == 1 and int(v[0]) == 1_000_000
    w.close()
    rng = np.random.default_rng(3)
    distinct = wide(rng.integers(0, 1 << 64, 190_000, dtype=np.uint64, endpoint=False), rng.integers(0, 4, 190_000, dtype=np.uint64))
    sel = rng.integers(0, len(distinct), 1 << 20)
    w = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash="farm")
    w.insert_reduce_plus(torch.from_numpy(distinct[sel].view(np.int64)).cuda())
    cnt = np.bincount(sel, minlength=len(distinct))
    present = cnt > 0
    assert w.size() == int(present.sum())
    v, f = w.find_values(distinct)
    assert np.array_equal(f.astype(bool), present) and np.array_equal(v[present], cnt[present].astype(np.uint32))
    w.close()


def test_probe_overflow_leaves_table_unchanged():
    w = kh.hashmap_robinhood_doubling_wide(1024, 0.35, 0.9, hash="identity")
    same_home = wide(np.arange(200, dtype=np.uint64) << np.uint64(40), np.arange(200, dtype=np.uint64))
    assert w.insert(same_home[:100], np.arange(100, dtype=np.uint32)) == 100
    info, items, cap = w.export_info(), w.sorted_items(), w.capacity()
    with pytest.raises(kh.KhError) as e:
        w.insert(same_home[100:140], np.arange(40, dtype=np.uint32))
    assert e.value.status == K.KH_ERR_PROBE_OVERFLOW
    assert w.size() == 100 and w.capacity() == cap and np.array_equal(w.export_info(), info)
    after = w.sorted_items()
    assert np.array_equal(after[0], items[0]) and np.array_equal(after[1], items[1])
    with pytest.raises(kh.KhError) as e:
        w.insert_reduce_plus(np.concatenate([same_home[:100], same_home[100:140]]), np.ones(140, dtype=np.uint32))
    assert e.value.status == K.KH_ERR_PROBE_OVERFLOW
    after = w.sorted_items()
    assert np.array_equal(after[1], items[1])          # the sums of the existing keys were taken back
    w.close()


def test_linear_probe_wide_is_unsupported():
    import ctypes as C
    h = C.c_void_p()
    assert K.lib().kh_wide_create(C.byref(h), K.KH_KIND_LINEARPROBE, 1, 43, 128, 0.2, 0.6, 0) == K.KH_ERR_UNSUPPORTED


def test_scale_107m_keys_at_load_08():
    n = 107_374_184
    cap = 1 << 27
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    keys = torch.randint(0, 1 << 62, (n, 2), dtype=torch.int64, device="cuda", generator=g)     # (bit 62 of w1 clear: the absent keys set it)
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    w = kh.hashmap_robinhood_doubling_wide(cap, 0.35, 0.8)
    assert w.insert(keys, vals) == n
    assert w.size() == n and w.capacity() == cap
    v, f = w.find_values(keys)
    assert bool(f.bool().all()) and bool((v == vals).all())
    del v, f
    absent = torch.randint(0, 1 << 62, (10_000_000, 2), dtype=torch.int64, device="cuda", generator=g)
    absent[:, 1] |= (1 << 62)
    assert int(w.count(absent).sum()) == 0
    del absent
    homes = (kh.hash_batch_wide(keys, "murmur3avx64", 43) & (cap - 1)).cpu().numpy()
    del keys, vals
    info = rh_info_model(homes, cap)
    hist = np.bincount(info[info >= 0x80] & 0x7F, minlength=128)
    assert np.array_equal(w.displacement_histogram(), hist.astype(np.uint64))
    w.close()
