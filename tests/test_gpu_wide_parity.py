"""GPU: the 16-byte-key Robin Hood table (kh_wide_*) pinned to the CPU model of oracle/wide_model.py, call by call and bit-exactly:
scalars, the info array, WHICH key sits in which slot (up to the order among the keys of one home), values, and count / find_values /
find from host and from device memory.  The model is independent of the library: capacities from the 64-bit CPU oracle over surrogate
keys, values from a dict, the layout from the canonical Robin Hood scan over homes hashed on the CPU (tests/test_wide_model.py
validates it without a GPU).  The cases aim at the edges of the kw_* kernels: wrap-around over one and several chunks, a run over a
chunk boundary, probe distance 127 and the refused 129th key, the class split of kw_dedup, kw_gather_new, the three shapes of
kw_for_each_old, several doublings pending, several passes per call and the streamed insert.

Identity-hash keys are written home | (tag << 40) in w0 with a distinct w1: the home is chosen, the keys differ in both words."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle.wide_model import HASH_IDS, WideModel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
POISON = 0xDEADBEEFDEADBEEF
HASHES = ("identity", "murmur3avx64", "murmur", "farm")


def dk(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 2).view(np.int64)).cuda()


def dv(vals):
    return None if vals is None else torch.from_numpy(np.ascontiguousarray(vals, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy()


def u64(*x):
    return np.array(x, dtype=np.uint64)


def rand_u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)


_tag = [0]


def homed(homes, w1=None):
    """identity-hash keys with the given homes: w0 = home | (tag << 40), tags never repeat; w1 distinct (tag * odd constant) unless given"""
    homes = np.asarray(homes, dtype=np.uint64)
    tags = np.arange(_tag[0] + 1, _tag[0] + 1 + len(homes), dtype=np.uint64)
    _tag[0] += len(homes)
    w1 = tags * np.uint64(0x9E3779B97F4A7C15) if w1 is None else np.asarray(w1, dtype=np.uint64)
    return np.ascontiguousarray(np.stack([homes | (tags << np.uint64(40)), w1], axis=1))


def check_hashes(hname, seed, keys):
    """kh.hash_batch_wide (host and device input) equals the oracle's CPU hash of the 16 key bytes"""
    want = O.hash16_batch(HASH_IDS[hname], seed, keys)
    assert np.array_equal(kh.hash_batch_wide(keys, hname, seed), want)
    assert np.array_equal(host(kh.hash_batch_wide(dk(keys), hname, seed)).view(np.uint64), want)


def check_state(g, m, queries):
    """the table equals the model: scalars and layout, slot contents, queries from host and device memory"""
    cap = m.capacity()
    assert (g.size(), g.capacity()) == (m.size(), cap)
    info = g.export_info()
    assert np.array_equal(info, m.export_info())
    assert np.array_equal(g.displacement_histogram(), m.displacement_histogram())
    gk, gv = g.sorted_items()
    mk, mv = m.sorted_items()
    assert np.array_equal(gk, mk) and np.array_equal(gv, mv)
    # slot contents: to_vector() lists the occupied slots in slot order (kh_to_vector: flags per slot, stable compaction); the key in
    # occupied slot s at distance d must have its home at (s - d) mod capacity -- free is only the order among the keys of one home
    tk, tv = g.to_vector()
    occ = np.flatnonzero(info >= 0x80)
    assert len(occ) == len(tk) == m.size()
    if len(occ):
        d = (info[occ] & 0x7F).astype(np.int64)
        assert np.array_equal(m.homes(tk).astype(np.int64), (occ - d) % cap)
        sv, sf = m.find_values(tk)
        assert sf.all() and np.array_equal(sv, tv)
    # queries, once as a numpy array and once as a CUDA tensor
    q = np.ascontiguousarray(queries, dtype=np.uint64).reshape(-1, 2)
    dq = dk(q)
    mc = m.count(q)
    ch, cd = g.count(q), host(g.count(dq))
    assert np.array_equal(ch, mc) and np.array_equal(cd, mc)
    mvals, mfound = m.find_values(q)
    hv, hf = g.find_values(q)
    dvv, dff = g.find_values(dq)
    assert np.array_equal(hf, mfound) and np.array_equal(hv, mvals)
    assert np.array_equal(host(dff), mfound) and np.array_equal(host(dvv).view(np.uint32), mvals)
    fk, fv = m.find(q)
    hk, hvv = g.find(q)
    dkk, dvv2 = g.find(dq)
    assert np.array_equal(hk, fk) and np.array_equal(hvv, fv)
    assert np.array_equal(host(dkk).view(np.uint64), fk) and np.array_equal(host(dvv2).view(np.uint32), fv)


def both(g, m, op, *args, device=False):
    """one member call on the model and on the table; the return values agree, and what the model refuses (probe overflow) the table
    refuses with KH_ERR_PROBE_OVERFLOW.  device: the batch arguments are CUDA tensors"""
    gargs = args
    if device and op in ("insert", "insert_reduce_plus", "erase"):
        gargs = (dk(args[0]),) + tuple(dv(a) for a in args[1:])
    try:
        want = getattr(m, op)(*args)
    except RuntimeError:                      # the oracle's rehash threw std::logic_error
        with pytest.raises(kh.KhLogicError):
            getattr(g, op)(*gargs)
        return None
    if m.probe_overflow:
        with pytest.raises(kh.KhError) as e:
            getattr(g, op)(*gargs)
        assert e.value.status == K.KH_ERR_PROBE_OVERFLOW, e.value
        return None
    got = getattr(g, op)(*gargs)
    assert got == want, (op, got, want)
    return got


def pair(cap, mn, mx, hname, seed=43, cls=None):
    g = (cls or kh.hashmap_robinhood_doubling_wide)(cap, mn, mx, hash=hname, seed=seed)
    return g, WideModel(cap, mn, mx, hname, seed)


def make_pool(rng, n=30_000):
    """both words random; a quarter of the keys share w0 with another key and differ in w1 only; {0,0}, {M64,M64} and the poison
    pattern of KH_DEBUG_POISON are in it"""
    w0, w1 = rand_u64(rng, n), rand_u64(rng, n)
    w0[: n // 4] = w0[n // 4: 2 * (n // 4)]
    pool = np.ascontiguousarray(np.stack([w0, w1], axis=1))
    pool[-3:] = [[0, 0], [M64, M64], [POISON, POISON]]
    return pool


def make_vals(rng, n):
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    v[0::5] = 0
    v[1::5] = M32
    return v


def make_queries(rng, m, pool, extra=None):
    """present keys, never-inserted keys, and absent keys that differ from a present key in w1 only"""
    parts = [pool[rng.integers(0, len(pool), 300)], np.stack([rand_u64(rng, 100), rand_u64(rng, 100)], axis=1)]
    live = m.sorted_items()[0]
    if len(live):
        near = live[rng.integers(0, len(live), 200)].copy()
        parts.append(near.copy())
        near[:, 1] ^= np.uint64(1) << rng.integers(0, 64, len(near)).astype(np.uint64)
        parts.append(near)
    if extra is not None and len(extra):
        parts.append(extra)
    return np.ascontiguousarray(np.concatenate(parts))


# ---- 1. random operation sequences ---------------------------------------------------------------------------------------------------
OPS = ["insert"] * 4 + ["plus_vals"] * 3 + ["plus_ones"] * 2 + ["erase"] * 3 + ["reserve", "rehash_up", "rehash_down", "clear"]
SIZES = [0, 1, 7, 300, 2049, 20_000]
FIXED = {0: "insert", 1: "plus_vals", 2: "erase", 3: "plus_ones", 12: "rehash_down", 18: "reserve", 24: "clear", 25: "insert", 31: "rehash_up"}   # every
#         operation occurs in every sequence, on a loaded table; the other 31 calls are drawn


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("hname", HASHES)
def test_random_operation_sequences(oracle, hname, seed):
    """40 calls drawn from insert, both insert_reduce_plus forms, erase, reserve, rehash up / down and clear; batches of 0 .. 20000
    records with duplicates, host and device input alternating; check_state after every call.  Under the identity hash the homes are
    the low bits of random w0s: no home collects 128 keys, the model never refuses"""
    rng = np.random.default_rng(1000 * seed + HASHES.index(hname))
    pool = make_pool(rng)
    g, m = pair(128, 0.35, 0.8, hname, 43 + seed)
    check_hashes(hname, 43 + seed, pool)
    seen = set()
    for step in range(40):
        op = FIXED.get(step) or OPS[int(rng.integers(0, len(OPS)))]
        n = 20_000 if step in (0, 1, 25) else SIZES[int(rng.integers(0, len(SIZES)))]
        keys = pool[rng.integers(0, len(pool), n)]                      # duplicates included; an erase batch also holds absent keys
        vals = make_vals(rng, n)
        device = bool(step & 1)
        if op == "insert":
            both(g, m, "insert", keys, vals, device=device)
        elif op == "plus_vals":
            both(g, m, "insert_reduce_plus", keys, vals, device=device)
        elif op == "plus_ones":
            both(g, m, "insert_reduce_plus", keys, device=device)
        elif op == "erase":
            never = np.stack([rand_u64(rng, n // 4), rand_u64(rng, n // 4)], axis=1)
            both(g, m, "erase", np.ascontiguousarray(np.concatenate([keys, never, keys[: n // 8]])), device=device)
        elif op == "reserve":
            both(g, m, "reserve", int(rng.integers(0, 50_000)))
        elif op == "rehash_up":
            both(g, m, "rehash", min(m.capacity() * int(rng.choice([2, 8])), 1 << 16))
        elif op == "rehash_down":
            both(g, m, "rehash", max(1, m.capacity() // int(rng.choice([2, 4, 64]))))
        else:
            both(g, m, "clear")
        assert not m.probe_overflow
        seen.add(op)
        check_state(g, m, make_queries(rng, m, pool, keys[:200]))
    assert seen == set(OPS), seen
    g.close(); m.close()


# ---- 2. / 3. runs that wrap around the table and runs that cross a chunk boundary (identity hash) ------------------------------------
def run_erase_reinsert(g, m, keys, vals, absent, more_home):
    """the keys go in in two batches (host, device); every second key of the run is erased; ten more keys of one home follow"""
    rng = np.random.default_rng(len(keys))
    o = rng.permutation(len(keys))
    keys, vals = keys[o], vals[o]
    h = len(keys) // 2
    q = np.ascontiguousarray(np.concatenate([keys, absent]))
    both(g, m, "insert", keys[:h], vals[:h])
    check_state(g, m, q)
    both(g, m, "insert", np.ascontiguousarray(np.concatenate([keys[h:], keys[:7]])), np.concatenate([vals[h:], vals[:7] + np.uint32(1)]), device=True)
    assert not m.probe_overflow and m.size() == len(keys)
    check_state(g, m, q)
    order = np.lexsort((keys[:, 1], m.homes(keys)))                   # along the run: by home
    both(g, m, "erase", np.ascontiguousarray(keys[order][::2]), device=True)
    check_state(g, m, q)
    more = homed(np.full(10, more_home))
    both(g, m, "insert_reduce_plus", np.ascontiguousarray(np.concatenate([more, more[:3]])), np.arange(13, dtype=np.uint32))
    assert not m.probe_overflow
    check_state(g, m, np.ascontiguousarray(np.concatenate([q, more])))


@pytest.mark.parametrize("cap", [1024, 8192])
def test_wrap_around(oracle, cap):
    """homes cap-40 .. cap-1 hold three keys each, homes 0 .. 30 two each: the run wraps from the last slot to slot 0 -- inside one
    chunk at 1024, from the last of four chunks into the first (xcarry) at 8192"""
    g, m = pair(cap, 0.35, 0.9, "identity")
    keys = homed(np.concatenate([np.repeat(np.arange(cap - 40, cap), 3), np.repeat(np.arange(0, 31), 2)]))
    vals = np.arange(len(keys), dtype=np.uint32) * np.uint32(2654435761)
    absent = homed([cap - 1, cap - 1, cap - 2, 0, 0, 1, 1, 31, cap - 41])
    check_hashes("identity", 43, keys)
    run_erase_reinsert(g, m, keys, vals, absent, cap - 1)
    info = g.export_info()
    assert info[0] > 0x80 and info[cap - 1] >= 0x80                  # the run still wraps
    g.close(); m.close()


def test_chunk_boundary(oracle):
    """capacity 8192 (chunks of 2048 slots): a dense run over the boundary 2047 | 2048.  120 keys at home 2047 plus four at each home
    2040 .. 2060 cannot be laid out (the keys of home 2047 alone would reach distance 28 + 124 - 1 - 7 = 144): model and table refuse
    that batch.  With 60 keys at home 2047 the largest distance is 123 (home 2060): that batch goes in, then erase and re-insert"""
    g, m = pair(8192, 0.35, 0.9, "identity")
    four = homed(np.repeat(np.arange(2040, 2061), 4))
    at2047 = homed(np.full(120, 2047))
    absent = homed([2047, 2047, 2046, 2048, 2039, 2061, 2062])
    check_hashes("identity", 43, at2047)
    big = np.ascontiguousarray(np.concatenate([at2047, four]))
    both(g, m, "insert", big, np.arange(len(big), dtype=np.uint32))
    assert m.probe_overflow and m.size() == 0
    check_state(g, m, np.ascontiguousarray(np.concatenate([big, absent])))
    keys = np.ascontiguousarray(np.concatenate([at2047[:60], four]))
    vals = np.arange(len(keys), dtype=np.uint32) + np.uint32(0xFFFFFF00)
    run_erase_reinsert(g, m, keys, vals, absent, 2047)
    g.close(); m.close()


# ---- 4. probe distance 127 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("home", [500, 501])
def test_probe_distance_limit(oracle, home):
    """128 keys of one home (even / odd: kw_find reads slot pairs from the home): the last sits at distance 127; the 129th key is
    refused by insert and by insert_reduce_plus, whose sums into the 128 present keys are taken back"""
    g, m = pair(1024, 0.35, 0.9, "identity")
    keys = homed(np.full(140, home))
    vals = make_vals(np.random.default_rng(home), 140)
    absent = homed([home, home, home - 1, home - 1, home + 1, home + 1, home + 127, home + 128])
    q = np.ascontiguousarray(np.concatenate([keys, absent]))
    check_hashes("identity", 43, keys)
    both(g, m, "insert", keys[:64], vals[:64])
    check_state(g, m, q)
    both(g, m, "insert", keys[64:128], vals[64:128], device=True)
    assert not m.probe_overflow
    check_state(g, m, q)
    info = g.export_info()
    assert info[home + 127] == 0xFF and info[home] == 0x80 and info[home + 128] == 0
    assert g.count(keys[:128]).all() and host(g.count(dk(keys[:128]))).all()          # the key at distance 127 among them
    both(g, m, "insert", keys[128:129], vals[128:129])                                         # the 129th key
    assert m.probe_overflow
    check_state(g, m, q)
    both(g, m, "insert_reduce_plus", keys[:129], vals[:129], device=True)
    assert m.probe_overflow
    check_state(g, m, q)
    both(g, m, "insert_reduce_plus", keys[:129])
    assert m.probe_overflow
    check_state(g, m, q)
    both(g, m, "erase", np.ascontiguousarray(keys[5:125:12]))
    assert m.size() == 118
    check_state(g, m, q)
    both(g, m, "insert", keys[128:138], vals[128:138], device=True)
    assert not m.probe_overflow and m.size() == 128
    check_state(g, m, q)
    g.close(); m.close()


# ---- 5. kw_dedup: more distinct keys in one partition than its LDS staging holds ------------------------------------------------------
@pytest.mark.parametrize("preload", [0, 500])
def test_dedup_class_split(oracle, preload):
    """2000 distinct keys with homes 0 .. 1999, three occurrences each, shuffled: the batch of 6000 records is partitioned for capacity
    8192, all of it into the partition of chunk 0 -- more than 1536 distinct keys, two classes.  insert (first wins), then
    insert_reduce_plus of the same records (every key present: the update list of both classes)"""
    rng = np.random.default_rng(50 + preload)
    g, m = pair(4096, 0.35, 0.8, "identity")
    keys = homed(np.arange(2000))
    sel = rng.permutation(np.repeat(np.arange(2000), 3))
    vals = make_vals(rng, len(sel))
    q = np.ascontiguousarray(np.concatenate([keys, homed(np.arange(0, 2100, 7))]))
    check_hashes("identity", 43, keys)
    if preload:
        both(g, m, "insert", keys[rng.permutation(2000)[:preload]], np.arange(preload, dtype=np.uint32) + np.uint32(5))
        check_state(g, m, q)
    assert both(g, m, "insert", keys[sel], vals, device=True) == 2000 - preload
    check_state(g, m, q)
    assert both(g, m, "insert_reduce_plus", keys[sel], vals) == 0
    check_state(g, m, q)
    assert both(g, m, "insert_reduce_plus", keys[sel], device=True) == 0
    check_state(g, m, q)
    g.close(); m.close()


def test_dedup_class_split_then_refusal(oracle):
    """5000 distinct keys whose homes all lie in chunk 0 of a capacity-8192 table that holds 300 keys: four or more classes in
    kw_dedup, then a layout no Robin Hood table has (2048 homes, 5000 keys).  The call is refused with KH_ERR_PROBE_OVERFLOW -- not
    KH_ERR_HIP, the de-duplication itself succeeded -- and the table is the one before the call"""
    rng = np.random.default_rng(55)
    g, m = pair(8192, 0.35, 0.9, "identity")
    old = homed(rng.integers(0, 8192, 300))
    both(g, m, "insert", old, make_vals(rng, 300))
    batch = homed(rng.integers(0, 2048, 5000))
    q = np.ascontiguousarray(np.concatenate([old, batch[:500]]))
    check_state(g, m, q)
    both(g, m, "insert", batch, make_vals(rng, 5000), device=True)                 # (both() asserts the status)
    assert m.probe_overflow
    check_state(g, m, q)
    both(g, m, "insert_reduce_plus", np.ascontiguousarray(np.concatenate([batch, old])), make_vals(rng, 5300))
    assert m.probe_overflow
    check_state(g, m, q)
    g.close(); m.close()


# ---- 6. capacity far below the partitioning capacity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("plus", [False, True])
def test_capacity_far_below_partitioning_capacity(oracle, plus):
    """40000 records over 400 distinct keys into an empty table of capacity 128: partitioned for 65536 buckets (32 partitions), laid
    out at 512 (one chunk) -- PB - k_new = 5: the per-partition lists are gathered (kw_gather_new)"""
    rng = np.random.default_rng(60 + plus)
    g, m = pair(128, 0.35, 0.8, "farm")
    distinct = make_pool(rng, 400)
    keys = distinct[rng.integers(0, 400, 40_000)]
    vals = make_vals(rng, 40_000)
    check_hashes("farm", 43, distinct)
    both(g, m, "insert_reduce_plus" if plus else "insert", keys, vals, device=True)
    assert m.capacity() == 512
    q = make_queries(rng, m, distinct)
    check_state(g, m, q)
    both(g, m, "insert_reduce_plus" if plus else "insert", keys, vals)              # every key present
    check_state(g, m, q)
    g.close(); m.close()


# ---- 7. re-layout shapes -------------------------------------------------------------------------------------------------------------
def test_relayout_shapes(oracle):
    """kw_for_each_old with fewer old chunks than new (4096 -> 16384), more (16384 -> 4096) and several chunks down to one
    (4096 -> 1024 after an erase); rehash(1024) with 2500 keys re-doubles to 4096 as the oracle's does"""
    rng = np.random.default_rng(70)
    g, m = pair(1024, 0.35, 0.8, "murmur3avx64")
    pool = make_pool(rng, 2500)
    check_hashes("murmur3avx64", 43, pool)
    both(g, m, "insert", pool, make_vals(rng, 2500), device=True)
    q = make_queries(rng, m, pool)
    check_state(g, m, q)
    for b, cap in ((1024, 4096), (16_384, 16_384), (4096, 4096), (3000, 4096), (1, 4096)):
        both(g, m, "rehash", b)
        assert m.capacity() == cap
        check_state(g, m, q)
    both(g, m, "erase", pool[700:])
    assert m.size() == 700
    check_state(g, m, q)
    both(g, m, "rehash", 1024)
    assert m.capacity() == 1024
    check_state(g, m, q)
    both(g, m, "reserve", 5000)
    assert m.capacity() == 8192
    check_state(g, m, q)
    g.close(); m.close()


# ---- 8. more than one doubling pending -----------------------------------------------------------------------------------------------
def test_more_than_one_doubling_pending(oracle):
    """the wide mirror of test_gpu_parity.test_more_than_one_doubling_pending, batch form: 20000 keys at capacity 32768, then max load
    0.25 (max_load(65536) = 16384 < 20000): ONE batch insert re-doubles inside the rehash and ends at 131072"""
    rng = np.random.default_rng(80)
    g, m = pair(128, 0.35, 0.8, "murmur")
    pool = make_pool(rng, 20_001)
    vals = make_vals(rng, 20_001)
    both(g, m, "insert", pool[:20_000], vals[:20_000], device=True)
    assert m.capacity() == 32_768
    g.set_max_load_factor(0.25); m.set_max_load_factor(0.25)
    q = make_queries(rng, m, pool)
    check_state(g, m, q)
    b = np.ascontiguousarray(np.concatenate([pool[:3], pool[20_000:]]))
    assert both(g, m, "insert", b, np.concatenate([vals[:3] + np.uint32(9), vals[20_000:]]), device=True) == 1
    assert m.capacity() == 131_072
    check_state(g, m, q)
    g.close(); m.close()


# ---- 9. several passes per call ------------------------------------------------------------------------------------------------------
def child_several_passes():
    """runs in a fresh process with KH_MAX_PASS_RECORDS=1024 (read when the library is loaded)"""
    rng = np.random.default_rng(90)
    pool = make_pool(rng, 6000)
    g, m = pair(128, 0.35, 0.8, "murmur3avx64")
    sel = rng.integers(0, 3000, 9000)
    sel[1020:1030] = sel[1010:1020]                                     # duplicates on both sides of the first pass boundary
    sel[2040:2050] = sel[10:20]
    sel[-5:] = sel[:5]
    both(g, m, "insert", pool[sel], make_vals(rng, 9000), device=True)
    q = make_queries(rng, m, pool)
    check_state(g, m, q)
    sel = rng.integers(0, 6000, 5000)
    sel[1020:1030] = sel[1010:1020]
    both(g, m, "insert_reduce_plus", pool[sel], make_vals(rng, 5000))
    check_state(g, m, q)
    both(g, m, "insert_reduce_plus", pool[sel], device=True)
    check_state(g, m, q)
    g.close(); m.close()
    print("several passes ok")


def test_several_passes_per_call(oracle):
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_wide_parity as T; T.child_several_passes()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KH_MAX_PASS_RECORDS="1024"), capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert r.returncode == 0 and "several passes ok" in r.stdout, r.stdout + r.stderr


# ---- 10. streamed insert -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plus", [False, True])
@pytest.mark.parametrize("pieces", [1, 2, 5, 16])
def test_streamed_insert(oracle, pieces, plus):
    """the pool of case 1 (and 5000 repeats) fed in 1, 2, 5 and 16 pieces of unequal length: the result is the model's single insert of
    the concatenation; an aborted streamed insert leaves the table as it was"""
    rng = np.random.default_rng(100 + pieces)
    pool = make_pool(rng)
    keys = np.ascontiguousarray(np.concatenate([pool[:2000], pool[rng.permutation(len(pool))], pool[rng.integers(0, len(pool), 3000)]]))
    vals = make_vals(rng, len(keys))
    g, m = pair(128, 0.35, 0.8, "murmur3avx64", cls=kh.hashmap_robinhood_doubling_wide_stream)
    both(g, m, "insert", keys[:2000], vals[:2000])
    q = make_queries(rng, m, pool)
    cuts = [0] + sorted(rng.integers(0, len(keys), pieces - 1).tolist()) + [len(keys)]
    device = bool(pieces & 1)
    held = []

    def feed(upto):
        for a, b in list(zip(cuts[:-1], cuts[1:]))[:upto]:
            k, v = keys[a:b], vals[a:b]
            if device:
                k, v = dk(k), dv(v)
                held.append((k, v))
            g.insert_feed(k, v)

    g.insert_begin(len(keys), reduce_plus=plus)
    feed(max(1, pieces // 2))
    g.insert_abort()
    check_state(g, m, q)                                                # the model before the call
    g.insert_begin(len(keys), reduce_plus=plus)
    feed(pieces)
    got = g.insert_end()
    want = m.insert_reduce_plus(keys, vals) if plus else m.insert(keys, vals)
    assert got == want and not m.probe_overflow
    check_state(g, m, q)
    g.close(); m.close()
