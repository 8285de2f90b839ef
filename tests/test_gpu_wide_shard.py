"""GPU: the two device-side pieces the sharded layer needs for 16-byte keys.
kh_wide_shard_permute -- the stable partition by destination rank -- against numpy (hash_batch_wide reduced mod p, stable argsort), and
with it kh_shard_permute, the same kernels instantiated for 8-byte keys (against the CPU oracle's hash_batch reduced mod p);
the streamed insert of the wide table (kh_wide_insert_begin_ex / feed / end / abort) against ONE plain insert of the concatenated
pieces: same return value, size, capacity, canonical Robin Hood layout (export_info, byte-equal) and items."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from kmerhash_amd.dist import DIST_SEED  # noqa: E402
from kmerhash_amd.table import _hash_id  # noqa: E402

HASHES = ("murmur3avx64", "murmur", "farm", "identity")
SIZES = (0, 1, 4095, 4096, 4097, 10**6 + 3)             # 16-byte keys: a tile is 2048 keys
SIZES_P9 = SIZES[:-1] + (2047, 2048, 2049, 6147)        # ... its edges and one multi-tile size, for p = 9
NARROW_SIZES = (0, 1, 4095, 4096, 4097, 12_291)         # 8-byte keys: the edges of a 4096-key tile and one multi-tile size
# 8 / 9: the last p of the LDS-staged kernel / the first of the generic one (and no power of two); 64: KH_SHARD_MAXR
RANKS = (1, 2, 3, 4, 5, 8, 9, 16, 64)
WIDTHS = [pytest.param(2, id="wide"), pytest.param(1, id="narrow")]
# (the 16-byte cases keep the ids they had before the 8-byte ones joined them)
WIDTH_HASH = [pytest.param(2, h, id=h) for h in HASHES] + [pytest.param(1, h, id="narrow-" + h) for h in HASHES]
GUARD = 64
SENT_K, SENT_V = -0x0123456789ABCDEF, 0x5A5A5A5A


def dev_keys(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev_vals(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def random_wide(rng, n, pool=None):
    if pool is not None:
        return pool[rng.integers(0, len(pool), n)]
    return rng.integers(0, 1 << 63, (n, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 2), dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# kh_wide_shard_permute / kh_shard_permute (kw: 64-bit words per key)
# ---------------------------------------------------------------------------------------------------------------------------------
def shard_fn(kw):
    return K.lib().kh_wide_shard_permute if kw == 2 else K.lib().kh_shard_permute


def permute(hash, p, dk, dv, n, count_only=False, kw=2):
    """-> (status, out keys (n, 2) or (n,) | None, out vals | None, counts[p]); the outputs carry GUARD sentinel rows behind them"""
    ok = torch.full((n + GUARD, 2) if kw == 2 else (n + GUARD,), SENT_K, dtype=torch.int64, device="cuda")
    ov = torch.full((n + GUARD,), SENT_V, dtype=torch.int32, device="cuda")
    counts = (C.c_uint64 * max(p, 1))(*([77] * max(p, 1)))
    st = shard_fn(kw)(_hash_id(hash), DIST_SEED, p, dk.data_ptr() if n else None, dv.data_ptr() if (dv is not None and n) else None, n,
                      None if count_only else ok.data_ptr(), None if (count_only or dv is None) else ov.data_ptr(), counts, 0,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, ok, ov, [int(c) for c in counts]


@pytest.fixture(scope="module")
def shard_input():
    rng = np.random.default_rng(31)
    n = max(SIZES)
    keys = random_wide(rng, n)
    keys[1::5, 0] = keys[0::5, 0][: len(keys[1::5])]          # keys that share one word with a neighbour
    keys[2::5, 1] = keys[0::5, 1][: len(keys[2::5])]
    keys[50_000:50_600] = keys[7]                               # a run of one key: a whole wave for one rank
    vals = np.arange(n, dtype=np.uint32)
    return keys, vals, dev_keys(keys), dev_vals(vals)


@pytest.fixture(scope="module")
def narrow_shard_input():
    rng = np.random.default_rng(32)
    n = max(NARROW_SIZES)
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    keys[5_000:5_600] = keys[7]                                 # a run of one key: a whole wave for one rank
    vals = np.arange(n, dtype=np.uint32)
    return keys, vals, dev_keys(keys), dev_vals(vals)


@pytest.mark.parametrize("kw,hash", WIDTH_HASH)
def test_shard_permute_matches_numpy(request, oracle, kw, hash):
    keys, vals, dk, dv = request.getfixturevalue("shard_input" if kw == 2 else "narrow_shard_input")
    if kw == 2:
        h = kh.hash_batch_wide(dk, hash=hash, seed=DIST_SEED).cpu().numpy().view(np.uint64)
        assert np.array_equal(h[:1000], kh.hash_batch_wide(keys[:1000], hash=hash, seed=DIST_SEED))     # host and device hashes agree
    else:
        h = oracle.hash_batch(_hash_id(hash), DIST_SEED, keys)
    for p in RANKS:
        for n in (NARROW_SIZES if kw == 1 else SIZES_P9 if p == 9 else SIZES):
            r = (h[:n] & np.uint64(p - 1)) if p & (p - 1) == 0 else (h[:n] % np.uint64(p))
            r = r.astype(np.int64)
            order = np.argsort(r, kind="stable")
            exp_counts = np.bincount(r, minlength=p).tolist()
            if hash != "identity" and n >= 4095 and p <= 8:
                assert min(exp_counts) > 0
            for with_vals in (True, False):
                st, ok, ov, counts = permute(hash, p, dk, dv if with_vals else None, n, kw=kw)
                assert st == K.KH_OK, (kw, hash, p, n, st)
                assert counts == exp_counts, (kw, hash, p, n)
                assert np.array_equal(ok[:n].cpu().numpy().view(np.uint64), keys[:n][order]), (kw, hash, p, n, with_vals)
                assert bool((ok[n:] == SENT_K).all()), "wrote behind the key output"
                if with_vals:
                    assert np.array_equal(ov[:n].cpu().numpy().view(np.uint32), vals[:n][order]), (kw, hash, p, n)
                    assert bool((ov[n:] == SENT_V).all()), "wrote behind the value output"
                else:
                    assert bool((ov == SENT_V).all())
            st, ok, ov, counts = permute(hash, p, dk, None, n, count_only=True, kw=kw)
            assert st == K.KH_OK and counts == exp_counts, (kw, hash, p, n)
            assert bool((ok == SENT_K).all())


@pytest.mark.parametrize("kw", WIDTHS)
def test_shard_permute_argument_checks(request, kw):
    keys, vals, dk, dv = request.getfixturevalue("shard_input" if kw == 2 else "narrow_shard_input")
    for p in (0, 65):
        for n in (0, 5000):
            assert permute("murmur3avx64", p, dk, dv, n, kw=kw)[0] == K.KH_ERR_INVALID
    fn = shard_fn(kw)
    counts = (C.c_uint64 * 4)()
    s = torch.cuda.current_stream().cuda_stream
    out = torch.empty((100, 2), dtype=torch.int64, device="cuda")
    assert fn(1, DIST_SEED, 4, dk.data_ptr(), None, 100, out.data_ptr(), None, None, 0, s) == K.KH_ERR_INVALID      # no counts
    assert fn(7, DIST_SEED, 4, dk.data_ptr(), None, 100, out.data_ptr(), None, counts, 0, s) == K.KH_ERR_INVALID    # no such hash
    assert fn(1, DIST_SEED, 4, None, None, 100, out.data_ptr(), None, counts, 0, s) == K.KH_ERR_INVALID             # null keys
    assert fn(1, DIST_SEED, 4, dk.data_ptr(), dv.data_ptr(), 100, out.data_ptr(), None, counts, 0, s) == K.KH_ERR_INVALID   # values without room
    assert fn(1, DIST_SEED, 4, None, None, 0, None, None, counts, 0, s) == K.KH_OK and list(counts) == [0, 0, 0, 0]
    # 16-byte keys and their output are accessed 16 bytes at a time: a pointer 8 bytes off is refused, not dereferenced; 8-byte keys
    # have no such requirement
    off8 = K.KH_ERR_INVALID if kw == 2 else K.KH_OK
    assert fn(1, DIST_SEED, 4, dk.data_ptr() + 8, None, 100, out.data_ptr(), None, counts, 0, s) == off8
    assert fn(1, DIST_SEED, 4, dk.data_ptr(), None, 50, out.data_ptr() + 8, None, counts, 0, s) == off8
    assert fn(1, DIST_SEED, 4, dk.data_ptr() + 16, None, 99, out.data_ptr() + 16, None, counts, 0, s) == K.KH_OK


def test_backend_shard_is_the_c_call(shard_input):
    from kmerhash_amd.dist import WideGpuBackend
    keys, vals, dk, dv = shard_input
    be = WideGpuBackend(0)
    n = 100_001
    ok, ov, counts = be.shard(dk[:n], dv[:n], 3)
    st, ek, ev, ec = permute("murmur3avx64", 3, dk, dv, n)
    assert counts == ec == be.shard_counts(dk[:n], 3) and torch.equal(ok, ek[:n]) and torch.equal(ov, ev[:n])
    assert tuple(be.empty((5, 2), torch.int64).shape) == (5, 2) and be.empty(5, torch.uint8).shape[0] == 5
    with pytest.raises(ValueError):
        be.shard(dk[:n].reshape(-1), None, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# streamed insert
# ---------------------------------------------------------------------------------------------------------------------------------
def cut(n, weights):
    """piece boundaries for n keys cut by unequal weights (0 = an empty piece)"""
    w = np.asarray(weights, dtype=np.float64)
    b = np.floor(np.cumsum(w) / w.sum() * n).astype(np.int64)
    b[-1] = n
    return [0] + b.tolist()


FEEDS = {1: [1], 3: [5, 0, 2], 16: [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3]}


def stream_vs_plain(keys, vals, weights, plus, where, preload=None, hash="murmur3avx64", repeatable=False, with_vals=True, extra_empty=False):
    s = kh.hashmap_robinhood_doubling_wide_stream(128, hash=hash)
    p = kh.hashmap_robinhood_doubling_wide(128, hash=hash)
    if preload is not None:
        assert s.insert(*preload) == p.insert(*preload)
    n = len(keys)
    conv_k = dev_keys if where == "device" else (lambda a: a)
    conv_v = dev_vals if where == "device" else (lambda a: a)
    b = cut(n, weights)
    cap0 = s.capacity()
    s.insert_begin(n, reduce_plus=plus, repeatable=repeatable)
    held = []
    for i in range(len(weights)):
        kk = conv_k(keys[b[i]:b[i + 1]])
        vv = conv_v(vals[b[i]:b[i + 1]]) if with_vals else None
        held.append((kk, vv))
        s.insert_feed(kk, vv)
    if extra_empty:
        s.insert_feed(conv_k(keys[:0]), conv_v(vals[:0]) if with_vals else None)
    assert s.capacity() == cap0 and s.size() == p.size()          # nothing reaches the table before the end
    got = s.insert_end()
    fk, fv = conv_k(keys), (conv_v(vals) if with_vals else None)
    exp = p.insert_reduce_plus(fk, fv) if plus else p.insert(fk, fv)
    assert got == exp
    assert (s.size(), s.capacity()) == (p.size(), p.capacity())
    assert np.array_equal(s.export_info(), p.export_info())
    a, c = s.sorted_items(), p.sorted_items()
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    return s, p


@pytest.mark.parametrize("loaded", [False, True])
@pytest.mark.parametrize("plus", [False, True])
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("nfeeds", [1, 3, 16])
def test_streamed_insert_equals_one_insert(nfeeds, where, plus, loaded):
    rng = np.random.default_rng(1000 + nfeeds + (7 if plus else 0))
    pool = random_wide(rng, 90_000)
    n = 200_003
    keys = random_wide(rng, n, pool)                   # every key about twice: duplicates inside and between pieces
    keys[n - 50:] = keys[:50]                          # and late repeats of the first piece's first keys
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    preload = None
    if loaded:                                         # a table that already holds a third of the pool (and has doubled a few times)
        pk = pool[::3].copy()
        preload = (pk, np.arange(len(pk), dtype=np.uint32) + np.uint32(5))
    s, p = stream_vs_plain(keys, vals, FEEDS[nfeeds], plus, where, preload, extra_empty=nfeeds == 16)
    assert s.capacity() >= 128 * 1024                  # the batch crossed doublings
    s.close(); p.close()


@pytest.mark.parametrize("hash", ["murmur", "farm", "identity"])
def test_streamed_insert_other_hashes_counting_form_and_repeatable(hash):
    rng = np.random.default_rng(5)
    pool = random_wide(rng, 30_000)
    keys = random_wide(rng, 100_000, pool)
    vals = np.arange(len(keys), dtype=np.uint32)
    # vals = None with reduce_plus: every occurrence counts 1; KH_INS_REPEATABLE is accepted and the insert still is exact
    s, p = stream_vs_plain(keys, vals, FEEDS[3], True, "device", hash=hash, repeatable=True, with_vals=False)
    assert int(s.sorted_items()[1].astype(np.int64).sum()) == len(keys)
    s.close(); p.close()
    s, p = stream_vs_plain(keys, vals, FEEDS[16], False, "device", hash=hash, repeatable=True)
    s.close(); p.close()


def test_streamed_insert_small_and_empty_totals():
    rng = np.random.default_rng(6)
    keys = random_wide(rng, 40)
    vals = np.arange(40, dtype=np.uint32)
    for n in (0, 1, 40):
        for where in ("device", "host"):
            s, p = stream_vs_plain(keys[:n], vals[:n], [2, 0, 1], False, where)
            s.close(); p.close()


def test_streamed_insert_more_than_one_doubling_pending():
    """max load factor lowered under the current load: several doublings are due, the batch has no one-pass form and takes the
    collect-then-insert fall-back -- still ONE insert of the concatenation"""
    rng = np.random.default_rng(8)
    pre = random_wide(rng, 50_000)
    keys = np.concatenate([random_wide(rng, 60_000), pre[:10_000]])
    vals = np.arange(len(keys), dtype=np.uint32)
    s = kh.hashmap_robinhood_doubling_wide_stream(128)
    p = kh.hashmap_robinhood_doubling_wide(128)
    pv = np.arange(len(pre), dtype=np.uint32)
    assert s.insert(pre, pv) == p.insert(pre, pv)
    for t in (s, p):
        t.set_max_load_factor(0.15)
        t.set_min_load_factor(0.05)
    b = cut(len(keys), [4, 1, 0, 7])
    s.insert_begin(len(keys))
    for i in range(4):
        s.insert_feed(dev_keys(keys[b[i]:b[i + 1]]), dev_vals(vals[b[i]:b[i + 1]]))
    assert s.insert_end() == p.insert(dev_keys(keys), dev_vals(vals))
    assert (s.size(), s.capacity()) == (p.size(), p.capacity())
    assert np.array_equal(s.export_info(), p.export_info())
    a, c = s.sorted_items(), p.sorted_items()
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    s.close(); p.close()


def test_streamed_insert_at_scale():
    """2 * 10^7 keys in 4 device pieces into a loaded table: thousands of partitions, partitions above the one-class limit of the LDS
    fold, a doubling decided at the end"""
    rng = np.random.default_rng(77)
    n = 20_000_000
    pool = random_wide(rng, 12_000_000)
    keys = np.concatenate([pool, random_wide(rng, n - len(pool), pool)])       # every pool key at least once, two thirds of them again
    keys[-1000:] = keys[0]                                                      # and one key a thousand times
    vals = np.arange(n, dtype=np.uint32)
    pk = pool[:2_000_000][::-1].copy()
    s, p = stream_vs_plain(keys, vals, [3, 2, 4, 1], False, "device", preload=(pk, np.full(len(pk), 9, dtype=np.uint32)))
    assert s.size() == len(pool) and s.capacity() >= 1 << 24
    s.close(); p.close()


def test_streamed_insert_contract_errors():
    rng = np.random.default_rng(9)
    keys = random_wide(rng, 30_000)
    vals = np.arange(len(keys), dtype=np.uint32)
    dk, dv = dev_keys(keys), dev_vals(vals)
    s = kh.hashmap_robinhood_doubling_wide_stream(128)
    assert s.insert(dk[:5000], dv[:5000]) == 5000
    info0, items0 = s.export_info(), s.sorted_items()

    def invalid(fn, *a, **kw):
        with pytest.raises(kh.KhError) as e:
            fn(*a, **kw)
        assert e.value.status == K.KH_ERR_INVALID, e.value

    def untouched():
        assert np.array_equal(s.export_info(), info0)
        a = s.sorted_items()
        assert np.array_equal(a[0], items0[0]) and np.array_equal(a[1], items0[1])

    # feed / end without begin
    invalid(s.insert_feed, dk[:10], dv[:10])
    invalid(s.insert_end)
    s.insert_abort()                                  # (no-op without a streamed insert)
    # an unknown flag
    assert K.lib().kh_wide_insert_begin_ex(s._h, 10, 4) == K.KH_ERR_INVALID
    # between begin and end: every other mutating / workspace call is refused, begin included
    s.insert_begin(20_000)
    s.insert_feed(dk[5000:12_000], dv[5000:12_000])
    for fn, a in ((s.insert, (dk[:10], dv[:10])), (s.insert_reduce_plus, (dk[:10],)), (s.count, (dk[:10],)), (s.find_values, (dk[:10],)),
                  (s.find, (dk[:10],)), (s.erase, (dk[:10],)), (s.reserve, (100_000,)), (s.rehash, (1 << 18,)), (s.clear, ()), (s.to_vector, ()),
                  (s.displacement_histogram, ()), (s.insert_begin, (5,))):
        invalid(fn, *a)
    # first-wins needs values
    invalid(s.insert_feed, dk[12_000:12_010], None)
    # over-feeding
    invalid(s.insert_feed, dk[:13_001], dv[:13_001])
    # ending short closes the streamed insert with nothing inserted
    invalid(s.insert_end)
    untouched()
    invalid(s.insert_end)
    # abort after two feeds (one from the host): the table is as before, and usable
    s.insert_begin(20_000, reduce_plus=True)
    s.insert_feed(dk[5000:12_000], dv[5000:12_000])
    s.insert_feed(keys[12_000:20_000])
    s.insert_abort()
    untouched()
    assert s.insert(dk[5000:6000], dv[5000:6000]) == 1000 and s.size() == 6000
    # the stated feed limit: 16 non-empty pieces (empty ones do not count), KH_ERR_UNSUPPORTED beyond
    s.insert_begin(17 * 100)
    for i in range(16):
        s.insert_feed(dk[20_000 + 100 * i:20_100 + 100 * i], dv[20_000 + 100 * i:20_100 + 100 * i])
        s.insert_feed(dk[:0], dv[:0])
    with pytest.raises(kh.KhError) as e:
        s.insert_feed(dk[21_600:21_700], dv[21_600:21_700])
    assert e.value.status == K.KH_ERR_UNSUPPORTED
    s.insert_abort()
    assert s.size() == 6000
    # the base class has no streamed member (and a plain wide table is not disturbed by any of this)
    assert not hasattr(kh.hashmap_robinhood_doubling_wide, "insert_begin")
    s.close()


def test_feed_limit_does_not_depend_on_the_table_state():
    """the 17th non-empty feed is refused in the collect-then-insert form too (several doublings pending), as in the one-pass form"""
    rng = np.random.default_rng(10)
    keys = random_wide(rng, 40_000)
    vals = np.arange(len(keys), dtype=np.uint32)
    dk, dv = dev_keys(keys), dev_vals(vals)
    s = kh.hashmap_robinhood_doubling_wide_stream(128)
    assert s.insert(dk[:30_000], dv[:30_000]) == 30_000
    s.set_max_load_factor(0.15)
    s.set_min_load_factor(0.05)
    s.insert_begin(1700)
    for i in range(16):
        s.insert_feed(dk[30_000 + 100 * i:30_100 + 100 * i], dv[30_000 + 100 * i:30_100 + 100 * i])
        s.insert_feed(dk[:0], dv[:0])
    with pytest.raises(kh.KhError) as e:
        s.insert_feed(dk[31_600:31_700], dv[31_600:31_700])
    assert e.value.status == K.KH_ERR_UNSUPPORTED
    s.insert_abort()
    assert s.size() == 30_000
    s.close()


def _multipass_worker(q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["KH_MAX_PASS_RECORDS"] = "40000"            # read once, when the library is loaded
    try:
        rng = np.random.default_rng(12)
        pool = random_wide(rng, 120_000)
        keys = random_wide(rng, 300_000, pool)
        vals = np.arange(len(keys), dtype=np.uint32)
        for plus in (False, True):
            for where in ("device", "host"):
                s, p = stream_vs_plain(keys, vals, FEEDS[16], plus, where)
                assert s.size() == len(np.unique(keys, axis=0))
                s.close(); p.close()
        q.put("ok")
    except Exception:  # pragma: no cover
        import traceback
        q.put("FAIL: " + traceback.format_exc())


def test_streamed_insert_forced_multi_pass():
    """KH_MAX_PASS_RECORDS far below the batch: the streamed insert has no one-pass form, collects the pieces and inserts them in
    several passes -- as the plain insert does.  In a child process: the library reads the variable when it is loaded."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_multipass_worker, args=(q,))
    p.start()
    res = q.get(timeout=600)
    p.join(60)
    assert res == "ok", res
