"""CPU: the model of the 16-byte-key Robin Hood table (oracle/wide_model.py) validated without a GPU.  Under the identity hash with
w1 = 0 the model and the 64-bit oracle table are the same table: a seeded operation sequence must agree call by call.  The homes of
the model come from ora_hash16_batch, which is pinned here against the Python statements of the four hashes and against the host
build of include/kmerhash_amd/kh_hash.h (the program tests/test_wide_hash.py compiles)."""
import numpy as np
import pytest

from oracle.farm16 import farm_hash64_with_seed_16
from oracle.wide_model import HASH_IDS, WideModel
from test_wide_hash import M64, SEEDS, _b16, _keys, hashprog  # noqa: F401      (hashprog: the module fixture that compiles the host program)


def wide(w0):
    w0 = np.asarray(w0, dtype=np.uint64)
    return np.ascontiguousarray(np.stack([w0, np.zeros_like(w0)], axis=1))


def assert_same(m, o, q):
    assert (m.size(), m.capacity()) == (o.size(), o.capacity())
    assert not m.probe_overflow and not o.probe_overflow()
    assert np.array_equal(m.export_info(), o.export_info())
    assert np.array_equal(m.displacement_histogram(), o.displacement_histogram())
    mk, mv = m.sorted_items()
    ok, ov = o.sorted_items()
    assert np.array_equal(mk[:, 0], ok) and not mk[:, 1].any() and np.array_equal(mv, ov)
    assert np.array_equal(m.count(wide(q)), o.count(q))
    mvals, mf = m.find_values(wide(q))
    ovals, of = o.find(q)
    assert np.array_equal(mf, of) and np.array_equal(mvals[mf == 1], ovals[of == 1]) and not mvals[mf == 0].any()
    fk, fv = m.find(wide(q))
    ck, cv = o.find_compact(q)
    assert np.array_equal(fk[:, 0], ck) and np.array_equal(fv, cv)


def test_identity_w1_zero_equals_the_64bit_oracle(oracle):
    """60 seeded operations (insert, erase, reserve, rehash up and down, clear; sizes 0 .. 4000, duplicates included) on WideModel and
    on OracleTable(KIND_RH, identity): return value, size, capacity, info array, displacement histogram, sorted items and count / find
    of a mixed query batch agree after every call"""
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 1 << 63, 12_000, dtype=np.uint64)
    m = WideModel(128, 0.35, 0.8, "identity", 43)
    o = oracle.OracleTable(oracle.KIND_RH, 128, 0.35, 0.8, oracle.HASH_IDENTITY, 43)
    sizes = [0, 1, 5, 300, 2049, 4000]
    ops = ["insert"] * 4 + ["erase"] * 3 + ["reserve", "rehash_up", "rehash_down", "clear"]
    seen = set()
    for step in range(60):
        op = "insert" if step < 3 else ops[int(rng.integers(0, len(ops)))]
        if step == 40:
            op = "clear"
        n = sizes[int(rng.integers(0, len(sizes)))]
        keys = pool[rng.integers(0, len(pool), n)]                    # duplicates included
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if op == "insert":
            assert m.insert(wide(keys), vals) == o.insert(keys, vals)
        elif op == "erase":
            assert m.erase(wide(keys)) == o.erase(keys)
        elif op == "reserve":
            r = int(rng.integers(0, 12_000))
            m.reserve(r); o.reserve(r)
        elif op == "rehash_up":
            b = o.capacity() * int(rng.choice([2, 4]))
            m.rehash(b); o.rehash(b)
        elif op == "rehash_down":
            b = max(1, o.capacity() // int(rng.choice([2, 4, 16])))
            m.rehash(b); o.rehash(b)
        else:
            m.clear(); o.clear()
        seen.add(op)
        q = np.concatenate([keys[: n // 2], pool[rng.integers(0, len(pool), 500)], rng.integers(0, 1 << 63, 100, dtype=np.uint64)])
        assert_same(m, o, q)
    assert seen == set(ops)
    m.close(); o.close()


def test_overflow_is_refused_and_leaves_the_model_unchanged(oracle):
    """identity hash: the 129th key of one home would sit at distance 128; the flag is set, the call returns None, nothing changed"""
    m = WideModel(1024, 0.35, 0.9, "identity", 43)
    same_home = np.stack([np.uint64(500) | (np.arange(1, 131, dtype=np.uint64) << np.uint64(40)), np.arange(130, dtype=np.uint64)], axis=1)
    assert m.insert(same_home[:128], np.arange(128, dtype=np.uint32)) == 128 and not m.probe_overflow
    info = m.export_info()
    assert info[500 + 127] == 0xFF and info[500] == 0x80
    items = m.sorted_items()
    assert m.insert(same_home[128:], np.ones(2, dtype=np.uint32)) is None and m.probe_overflow
    assert m.insert_reduce_plus(same_home[:129]) is None and m.probe_overflow
    assert (m.size(), m.capacity()) == (128, 1024) and np.array_equal(m.export_info(), info)
    assert all(np.array_equal(a, b) for a, b in zip(m.sorted_items(), items))
    assert m.erase(same_home[:1]) == 1 and not m.probe_overflow
    assert m.insert(same_home[128:129], np.ones(1, dtype=np.uint32)) == 1 and m.size() == 128
    m.close()


@pytest.mark.parametrize("hname", ["identity", "murmur3avx64", "murmur", "farm"])
def test_hash16_batch_matches_statements_and_host_header(oracle, hashprog, hname):  # noqa: F811
    keys = _keys(256, 5)                                               # includes {0,0}, {M64,M64}, {1,0}, {0,1}
    arr = np.array(keys, dtype=np.uint64)
    col = ["identity", "murmur3avx64", "murmur", "farm"].index(hname)
    for seed in SEEDS:
        got = oracle.hash16_batch(HASH_IDS[hname], seed, arr).tolist()
        prog = hashprog([(a, b, seed, 0) for a, b in keys])
        for (a, b), g, p in zip(keys, got, prog):
            if hname == "identity":
                want = a
            elif hname == "murmur3avx64":
                x = oracle.murmur3_x86_128(_b16(a, b), seed); want = int(x[0]) | (int(x[1]) << 32)
            elif hname == "murmur":
                want = int(oracle.murmur3_x64_128(_b16(a, b), seed)[0])
            else:
                want = farm_hash64_with_seed_16(a, b, seed)
            assert g == want == p[col], (hname, a, b, seed)
    assert keys[1] == (M64, M64)
