"""GPU: the histogram-free two-pass partition with XCD-private write fronts (eight sub-slots and cursors per level-1 bucket in the
first pass, one bucket's tiles on one XCD in the second).  The smallest shape that reaches that branch: capacity 2^23 (2^12 partitions,
64 x 64 digits), a batch of 256 << 12 records or more.  Every result is checked against exact set arithmetic in numpy; the twin
run with KH_DISABLE_XCD_FRONTS=1 happens in a fresh child process (the switch is read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6_000_000
N2, NE = 1_000_000, 1_000_000
SEED = 61
CLS = {"rh": kh.hashmap_robinhood_doubling, "lp": kh.hashmap_linearprobe_doubling}
TILE = 8192


@pytest.fixture(autouse=True)
def sub_slots_at_small_shapes(monkeypatch):
    """the sub-slots are used from a mean fill of 4 tiles per sub-slot; these shapes have 1.4 (the library reads the variable at every call)"""
    monkeypatch.setenv("KH_XCD_FRONTS_MIN_TILES", "1")


def dev(a):
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


@pytest.fixture(scope="module")
def pool():
    """N + 1 keys of the first batch, then fresh keys for the later batches; all distinct.  Read-only."""
    return W.distinct_u64(N + 1 + 3_000_000, seed=SEED)


def sorted_pairs(k, v):
    o = np.argsort(k, kind="stable")
    return k[o], v[o]


def check_items(t, k, v):
    """the table holds exactly the pairs (k, v) (k distinct)"""
    a = t.sorted_items()
    b = sorted_pairs(k, v)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def check_found(t, k, v):
    fv, found = t.find_values(dev(k))
    assert bool(found.all())
    assert np.array_equal(fv.cpu().numpy().view(np.uint32), v)


@pytest.mark.parametrize("n", [N, N + 1])
@pytest.mark.parametrize("hash_", ["murmur3avx64", "farm"])
@pytest.mark.parametrize("kind", ["rh", "lp"])
def test_distinct_keys_then_second_batch_and_erase(pool, kind, hash_, n):
    """cases 1 and 2: distinct keys (n = 6 000 001: ragged last tile, 733 tiles -- no multiple of 8 or 64) through both tables and two
    hashes, 12-byte records; a second batch into the loaded table (16-byte records); an erase (8-byte records, slots whatever n is)"""
    keys = pool[:n]
    vals = np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(1)
    t = CLS[kind](128, 0.35, 0.8, hash=hash_)
    t.profile_enable(True)
    assert t.insert(dev(keys), dev(vals)) == n
    prof = t.profile()
    assert prof["k_part_scatter"][0] == 2 and "k_part_hist" not in prof, prof      # the histogram-free branch, accepted at once
    assert t.size() == n and t.capacity() == 1 << 23
    check_found(t, keys, vals)
    check_items(t, keys, vals)
    # second batch: 900 000 new keys and 100 000 the table holds (first value wins)
    k2 = np.concatenate([pool[N + 1:N + 1 + N2 - 100_000], keys[5:5 + 100_000]])
    v2 = np.arange(N2, dtype=np.uint32) + np.uint32(0x40000000)
    assert t.insert(dev(k2), dev(v2)) == N2 - 100_000
    allk = np.concatenate([keys, k2[:N2 - 100_000]]); allv = np.concatenate([vals, v2[:N2 - 100_000]])
    assert t.size() == len(allk) and t.capacity() == 1 << 24
    check_items(t, allk, allv)
    # erase: 800 000 present keys (both batches) and 200 000 absent ones
    ke = np.concatenate([keys[1000:1000 + 500_000], k2[:300_000], pool[N + 1 + N2:N + 1 + N2 + 200_000]])
    assert len(ke) == NE
    assert t.erase(dev(ke)) == 800_000
    keep = ~np.isin(allk, ke)
    assert t.size() == int(keep.sum())
    check_items(t, allk[keep], allv[keep])
    assert int(t.count(dev(ke)).sum().item()) == 0
    t.close()


def test_second_batch_large_enough_for_fixed_slots(pool):
    """a second batch of 256 << 13 records or more takes the histogram-free branch itself (16-byte records into a loaded table)"""
    keys = pool[:N]
    vals = np.arange(N, dtype=np.uint32)
    t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)
    assert t.insert(dev(keys), dev(vals)) == N
    n2 = 2_200_001
    k2 = np.concatenate([pool[N + 1:N + 1 + n2 - 50_000], keys[77:77 + 50_000]])
    v2 = np.arange(n2, dtype=np.uint32) + np.uint32(0x10000000)
    t.profile_enable(True)
    assert t.insert(dev(k2), dev(v2)) == n2 - 50_000
    prof = t.profile()
    assert "k_part_hist" not in prof, prof
    assert t.capacity() == 1 << 24
    check_items(t, np.concatenate([keys, k2[:n2 - 50_000]]), np.concatenate([vals, v2[:n2 - 50_000]]))
    t.close()


@pytest.mark.parametrize("kind", ["rh", "lp"])
def test_duplicates_the_sample_misses(pool, kind):
    """case 3: the duplicate sample reads every (n / 65536)-th key; a handful of repeats off that stride let the 12-byte attempt start,
    the build rejects it and the batch repeats with 16-byte records.  First value wins."""
    n = N
    keys = pool[:n].copy()
    stride = n // 65536
    for j in range(7):
        a, b = 91_000 * j * 9 + 7, 91_000 * j * 9 + 4001
        assert a % stride and b % stride and b < n
        keys[b] = keys[a]
    vals = np.arange(n, dtype=np.uint32) + np.uint32(11)
    uk, first = np.unique(keys, return_index=True)
    assert len(uk) == n - 7
    t = CLS[kind](128, 0.35, 0.8)
    t.profile_enable(True)
    assert t.insert(dev(keys), dev(vals)) == n - 7
    prof = t.profile()
    assert prof["k_part_scatter"][0] == 4, prof             # 12-byte attempt + 16-byte repeat, two passes each
    assert t.size() == n - 7 and t.capacity() == 1 << 23
    check_items(t, uk, vals[first])
    t.close()


@pytest.fixture(scope="module")
def x5():
    k, v = W.w3_kmers_5x(1_200_000, 5, seed=29)
    k.setflags(write=False); v.setflags(write=False)
    return k, v


def test_multiplicity_5_first_wins(x5):
    """case 4a: every key five times (16-byte records, slots widened by the sample's variance factor)"""
    keys, vals = x5
    uk, first = np.unique(keys, return_index=True)
    t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)
    t.profile_enable(True)
    assert t.insert(dev(keys), dev(vals)) == len(uk)
    prof = t.profile()
    assert prof["k_part_scatter"][0] == 2 and "k_part_hist" not in prof, prof
    assert t.size() == len(uk)
    check_items(t, uk, vals[first])
    t.close()


def test_multiplicity_5_counting_insert(x5):
    """case 4b: the same keys counted (8-byte records)"""
    keys, _ = x5
    uk, cnt = np.unique(keys, return_counts=True)
    t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)
    t.profile_enable(True)
    assert t.insert_reduce_plus(dev(keys)) == len(uk)
    prof = t.profile()
    assert prof["k_part_scatter"][0] == 2 and "k_part_hist" not in prof, prof
    check_items(t, uk, cnt.astype(np.uint32))
    t.close()


def test_sub_slot_overflow_repeats_with_exact_offsets(pool, monkeypatch):
    """case 5: hash = identity, so the level-1 digit of a key is known here: bits 11..16 of the key, reversed.  All keys of digit 0
    (n / 64 of them, eight sub-slots' worth) sit in the tiles that workgroups 0, 8, 16, ... take -- the eight-tile groups t % 64 < 8 of the
    swizzled order -- so sub-slot 0 of bucket 0 gets 6.7 times what it holds: the dump area takes the surplus, the flag is raised and
    the batch repeats with exact offsets.  The call returns normally and the table equals the input.
    (Crowding a third of the KEYS into one digit instead would crowd them into 1/64 of the table's buckets -- 2e6 keys for 131 072 home
    buckets, beyond the probe distance of 127 that the reference and the oracle allow; the key set here stays uniform and the sub-slot
    overflows through the order of the keys alone.)"""
    n = N
    k = pool[:n]
    d0 = ((k >> np.uint64(11)) & np.uint64(63)) == 0
    nd0 = int(d0.sum())
    assert 85_000 < nd0 < 102_000                                # ~ n / 64, against a sub-slot of ~14 000 records
    tile_of = np.arange(n) // TILE
    on_x0 = (tile_of % 64) < 8                                   # the tiles of workgroups with index & 7 == 0
    pos0 = np.flatnonzero(on_x0)[:nd0]
    assert len(pos0) == nd0
    rest = np.ones(n, dtype=bool); rest[pos0] = False
    keys = np.empty(n, dtype=np.uint64)
    keys[pos0] = k[d0]
    keys[rest] = k[~d0]
    vals = np.arange(n, dtype=np.uint32) ^ np.uint32(0x5555)
    t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="identity")
    t.profile_enable(True)
    assert t.insert(dev(keys), dev(vals)) == n                   # (returns: no error status)
    prof = t.profile()
    assert prof["k_part_scatter"][0] == 4 and "k_part_hist" in prof, prof      # fixed slots first, then exact offsets
    assert t.size() == n and t.capacity() == 1 << 23
    check_found(t, keys, vals)
    check_items(t, keys, vals)
    t.close()
    # the same batch with the sub-slots off for this shape (the default: 1.4 tiles per sub-slot are fewer than 4): nothing overflows, so the
    # overflow above was a sub-slot's
    monkeypatch.delenv("KH_XCD_FRONTS_MIN_TILES")
    t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="identity")
    t.profile_enable(True)
    assert t.insert(dev(keys), dev(vals)) == n
    prof = t.profile()
    assert prof["k_part_scatter"][0] == 2 and "k_part_hist" not in prof, prof
    check_items(t, keys, vals)
    t.close()


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import kmerhash_amd as kh
from kmerhash_amd import workloads as W
out, N, seed = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
pool = W.distinct_u64(N + 1, seed=seed)
res = {}
for hash_ in ("murmur3avx64", "farm"):
    for n in (N, N + 1):
        keys = pool[:n]
        vals = np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(1)
        t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash=hash_)
        ins = t.insert(torch.from_numpy(keys.view(np.int64)).cuda(), torch.from_numpy(vals.view(np.int32)).cuda())
        sk, sv = t.sorted_items()
        res["%s_%d_meta" % (hash_, n)] = np.array([ins, t.size(), t.capacity()], dtype=np.uint64)
        res["%s_%d_k" % (hash_, n)] = sk
        res["%s_%d_v" % (hash_, n)] = sv
        t.close()
np.savez(out, **res)
"""


def test_twin_run_with_fronts_disabled(pool, tmp_path):
    """case 6: case 1 again in a fresh process with KH_DISABLE_XCD_FRONTS=1: size, capacity and the sorted pairs equal the default run's
    (and, independently, the input)"""
    script = tmp_path / "twin.py"
    script.write_text(CHILD)
    out = str(tmp_path / "twin.npz")
    env = dict(os.environ, KH_DISABLE_XCD_FRONTS="1")
    r = subprocess.run([sys.executable, str(script), ROOT, out, str(N), str(SEED)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    twin = np.load(out)
    for hash_ in ("murmur3avx64", "farm"):
        for n in (N, N + 1):
            keys = pool[:n]
            vals = np.arange(n, dtype=np.uint32) * np.uint32(3) + np.uint32(1)
            t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash=hash_)
            ins = t.insert(dev(keys), dev(vals))
            sk, sv = t.sorted_items()
            assert np.array_equal(twin["%s_%d_meta" % (hash_, n)], np.array([ins, t.size(), t.capacity()], dtype=np.uint64))
            assert np.array_equal(twin["%s_%d_k" % (hash_, n)], sk) and np.array_equal(twin["%s_%d_v" % (hash_, n)], sv)
            ek, ev = sorted_pairs(keys, vals)
            assert np.array_equal(sk, ek) and np.array_equal(sv, ev) and ins == n and t.capacity() == 1 << 23
            t.close()
