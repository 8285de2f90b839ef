"""GPU: the bulk insert into an empty table as one kernel stream.  The host no longer reads the duplicate sample before it partitions:
it queues the attempt a clean sample would choose behind k_sample_dups (which also initialises the partition's cursors), the two
partition passes and the build test the sample's word and return at once if it is not zero, and the word reaches the host with the build's
control words.  The lean build adds its chunk counts to a few spread words and one tail launch (k_fused_tail) sums them, takes the carry
of the last chunk from its granule and places chunk 0.

Shape: the histogram-free partition and k_build_lean need more than 2^11 partitions and at least 256 records per partition, i.e. 2^12
chunks -- a table created with 2^23 buckets -- and 256 << 12 = 1 048 576 records (part_buffer_records; 1.1e6 keys into a fresh table of 128
buckets end at 2^21 buckets = 2^10 partitions and take exact offsets).  N = 1 200 001: 147 tiles, the last one ragged.  With
KH_XCD_FRONTS_MIN_TILES=0 the XCD sub-slots are used at this size (0.3 tiles per sub-slot).  Every result is compared with the CPU
oracle or with exact set arithmetic in numpy; every fall-back exercised here returns normally."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from stream_checks import assert_busy, late_inputs, side_stream, to_dev  # noqa: E402
from test_gpu_parity import check_state, dev  # noqa: E402

CAP = 1 << 23
N = 1_200_001
SEED = 97
CLS = {0: kh.hashmap_robinhood_doubling, 1: kh.hashmap_linearprobe_doubling}


@pytest.fixture(autouse=True)
def sub_slots_at_this_shape(monkeypatch):
    monkeypatch.setenv("KH_XCD_FRONTS_MIN_TILES", "0")


@pytest.fixture(scope="module")
def pool():
    """distinct keys: N for the batch, N more as the decoy of the stream test.  Read-only."""
    k = W.distinct_u64(2 * N, seed=SEED)
    k.setflags(write=False)
    return k


def vals_for(n, base=3):
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2 ** 32)).astype(np.uint32) + np.uint32(base)


def tables(kind=0, hash_="murmur3avx64", hash_id=O.HASH_MURMUR3_X86):
    return CLS[kind](CAP, 0.35, 0.8, hash=hash_), O.OracleTable(kind, CAP, 0.35, 0.8, hash_id, 43)


def check_items(t, k, v):
    a = t.sorted_items()
    o = np.argsort(k, kind="stable")
    assert np.array_equal(a[0], k[o]) and np.array_equal(a[1], v[o])


@pytest.mark.parametrize("kind", [0, 1], ids=["rh", "lp"])
def test_clean_batch_is_one_kernel_stream(pool, kind):
    """case 1: sample (+ cursors), two passes, the lean build, ONE tail launch -- chunk 0's placement, which stays a launch of its own
    because its 46 KB of LDS do not fit next to the lean build's 40 KB at four workgroups per CU; no k_fused_totals, no repeat"""
    keys, vals = pool[:N], vals_for(N)
    g, o = tables(kind)
    g.profile_enable(True)
    assert g.insert(dev(keys), dev(vals)) == o.insert(keys, vals) == N
    prof = g.profile()
    print(sorted((k, v[0]) for k, v in prof.items()))
    assert prof["k_part_scatter"][0] == 2 and prof["k_build_fused"][0] == 1 and prof["k_sample_dups"][0] == 1, prof
    assert prof["k_fused_tail"][0] == 1 and "k_fused_totals" not in prof and "k_part_hist" not in prof and "k_chunk_place" not in prof, prof
    check_state(g, o, kind)
    g.close()


@pytest.mark.parametrize("op", ["first", "update", "plus"])
def test_duplicates_the_sample_sees(pool, op):
    """case 2: 30 % of the keys repeated: the sample's word is not zero, the queued attempt returns at once, and the batch goes the way
    the host chose for such a sample before (slots widened by the sample's variance factor: two passes, no histogram)"""
    nd = 1_000_000
    rng = np.random.default_rng(5)
    keys = np.concatenate([pool[:nd], pool[:nd][rng.choice(nd, 300_000, replace=False)]])
    keys = keys[rng.permutation(len(keys))]
    vals = vals_for(len(keys), 9)
    g, o = tables()
    g.profile_enable(True)
    if op == "first":
        assert g.insert(dev(keys), dev(vals)) == o.insert(keys, vals) == nd
    elif op == "update":
        g.update(dev(keys), dev(vals))
        o.insert(keys, vals)
    else:
        assert g.insert_reduce(dev(keys), dev(vals), "plus") == nd
        o.insert(keys, vals)
    prof = g.profile()
    # (the two passes, the build and the tail launch that returned at once carry a label of their own; an update's attempt writes 16-byte
    #  records for the general one-launch build, which keeps its reduction launch, k_fused_totals, in front of the tail launch)
    assert prof["k_attempt_skipped"][0] == (5 if op == "update" else 4), prof
    assert prof["k_sample_dups"][0] == 1 and prof["k_part_scatter"][0] == 2, prof
    assert g.size() == o.size() == nd and g.capacity() == o.capacity() == CAP
    if op == "first":
        check_state(g, o, 0)
    else:
        uk, inv = np.unique(keys, return_inverse=True)
        if op == "update":
            exp = np.zeros(len(uk), dtype=np.uint32)
            exp[inv] = vals                                       # (in input order: the last occurrence stays)
        else:
            exp = np.bincount(inv, weights=vals.astype(np.float64), minlength=len(uk)).astype(np.uint64).astype(np.uint32)
        check_items(g, uk, exp)
        assert np.array_equal(g.export_info(), o.export_info())   # (the layout depends on the key set alone)
    g.close()


def test_one_duplicate_pair_the_sample_misses(pool):
    """case 3: the sample reads every (n // 65536)-th key; both copies lie off that stride, the build's own check raises its flag and
    the batch repeats with 16-byte records and exact offsets.  First value wins."""
    keys = pool[:N].copy()
    stride = N // 65536
    a, b = 700_003, 911_111
    assert a % stride and b % stride
    keys[b] = keys[a]
    vals = vals_for(N, 1)
    g, o = tables()
    g.profile_enable(True)
    assert g.insert(dev(keys), dev(vals)) == o.insert(keys, vals) == N - 1
    prof = g.profile()
    assert prof["k_sample_dups"][0] == 1 and prof["k_part_scatter"][0] == 4 and "k_part_hist" in prof, prof
    check_state(g, o, 0)
    g.close()


def test_slot_overflow_repeats_with_exact_offsets():
    """case 4: hash = identity over sorted keys 0 .. N-1: a tile's 8192 records share four partitions, every partition receives 2048
    records for a slot of about 430 -- the overflow word, read with the control words, sends the batch to exact offsets"""
    keys = np.arange(N, dtype=np.uint64)
    vals = vals_for(N, 2)
    g, o = tables(0, "identity", O.HASH_IDENTITY)
    g.profile_enable(True)
    assert g.insert(dev(keys), dev(vals)) == o.insert(keys, vals) == N
    prof = g.profile()
    assert prof["k_part_scatter"][0] == 4 and "k_part_hist" in prof, prof
    check_state(g, o, 0)
    g.close()


def test_chunk_0_takes_the_carry_of_the_last_chunk(pool):
    """case 5: hash = identity; three keys on each of the last 16 buckets run over the end of the table into chunk 0, which the tail
    launch places with that carry.  Accepted at once (no general path), info bytes equal the oracle's."""
    pile = (np.uint64(CAP - 16) + np.arange(16, dtype=np.uint64))[:, None] + (np.arange(1, 4, dtype=np.uint64) << np.uint64(32))[None, :]
    keys = np.concatenate([pool[:N - 48], pile.ravel()])
    assert len(np.unique(keys)) == N
    keys = keys[np.random.default_rng(8).permutation(N)]
    vals = vals_for(N, 4)
    g, o = tables(0, "identity", O.HASH_IDENTITY)
    g.profile_enable(True)
    assert g.insert(dev(keys), dev(vals)) == o.insert(keys, vals) == N
    prof = g.profile()
    assert prof["k_part_scatter"][0] == 2 and prof["k_fused_tail"][0] == 1 and "k_chunk_place" not in prof and "k_dedup" not in prof, prof
    info = o.export_info()
    assert info[CAP - 1] >= 0x80 and info[0] > 0x80 and info[15] > 0x80          # elements of the last chunk's buckets stand in chunk 0
    check_state(g, o, 0)
    g.close()


def test_insert_on_a_side_stream_behind_a_late_input(pool):
    """case 6: the keys and values are still being written on the caller's side stream when the insert is issued there"""
    keys, vals = pool[:N], vals_for(N, 6)
    dk, dv = pool[N:2 * N], vals_for(N, 7)
    s = side_stream()
    twin, _ = tables()
    with torch.cuda.stream(s):                                    # (the allocations of the real call are at hand afterwards)
        twin.insert(to_dev(dk), to_dev(dv))
    torch.cuda.synchronize()
    twin.close()
    g, o = tables()
    with torch.cuda.stream(s):
        bk, bv = late_inputs(s, (keys, dk), (vals, dv))
        assert_busy(s)
        got = g.insert(bk, bv)
    s.synchronize()
    assert got == o.insert(keys, vals) == N
    check_state(g, o, 0)
    g.close()
