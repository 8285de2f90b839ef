"""What a refused call leaves behind, on every insert path.

KH_ERR_PROBE_OVERFLOW is the one error a well-formed call can earn: a Robin Hood layout would need a probe distance of 128.  The
promise (include/kmerhash_amd.h) is a table exactly as before -- size, capacity, info bytes, items and values -- that
takes the next call.  Under the identity hash the failure is crafted at will: the keys home + ((i + 1) << 32) share the home bucket
`home` at every capacity, 128 of them stand at distances 0..127 (the last info byte 0xFF), 129 cannot be laid out.  Every case puts
such a pile on an ordinary spread background, so the table is a normal one everywhere else.  All comparisons are between integers.

snapshot / assert_unchanged (tests/refusal_checks.py) is the before/after check; assert_consistent judges a table whose key set the test did not choose by
tests/rh_canon.py (checked against both CPU oracles in tests/test_rh_canon.py).  Accepted batches are compared with the CPU oracle
(check_state of test_gpu_parity.py), the wide table with oracle/wide_model.py, reducer inserts with a twin table.

Shapes are the smallest that reach each kernel (the existing success test of each path), with two exceptions that the code forces:
  * k_build_lean needs 12-byte records, which only the histogram-free partition writes: more than 2^11 partitions and 256 records
    per partition, i.e. a capacity of 2^23 and 2^20 records.  300 000 distinct keys take the general form of k_build_fused (row
    build_distinct); row build_lean is 1 100 000 keys into a table created with 2^23 buckets.  Both forms carry the label k_build_fused; the
    lean row also asserts k_sample_dups and exactly two k_part_scatter launches (no repeat with exact offsets) in its accepted call.
  * k_insert_stream takes at most KH_IS_MAXR / 2 = 320 records per chunk on exact offsets: 60 000 records into 200 000 held at 2^19.
    200 000 records (row insert_z2, the table doubles) take the staging form.  Both carry the label k_insert_fused.
Which kernels refused is printed per case (pytest -s) from the profile of the refused call.  A fused kernel that raises the flag hands
the batch to the general path, whose re-layout (k_rebuild_fused where a loaded table keeps or doubles its capacity, k_chunk_place
otherwise: a build from empty, a capacity times four, fewer than two chunks) refuses again: the call's status comes from the last of them.  rehash() to a LARGER capacity never merges home buckets, so k_rebuild_fused is
shown refusing through the general path (rows general, insert_*), and rehash(2 cap) only with the accepted boundary."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402
from refusal_checks import assert_consistent, assert_unchanged, host_count, snapshot, thresholds  # noqa: E402
from rh_canon import canonical_info  # noqa: E402
from test_gpu_parity import check_state, dev  # noqa: E402
from test_gpu_reduce_ops import combined, draw_vals  # noqa: E402

RH, LP = kh.hashmap_robinhood_doubling, kh.hashmap_linearprobe_doubling
WIDE, WIDE_STREAM = kh.hashmap_robinhood_doubling_wide, kh.hashmap_robinhood_doubling_wide_stream
HOLE = 1000          # no background key has its home within this many buckets of a pile's home


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def pile(home, m, first=1):
    """m keys with the home bucket `home` at every capacity (identity hash)"""
    return np.uint64(home) + (np.arange(first, first + m, dtype=np.uint64) << np.uint64(32))


def spread(n, seed, cap, homes, hole=HOLE):
    """n distinct keys with uniform homes, none within `hole` buckets (circular, at capacity `cap` and so at every larger one) of the
    given pile homes"""
    k = W.splitmix64(W.distinct_u64(n + n // 8 + 64 * len(homes), seed=seed))
    h = (k & np.uint64(cap - 1)).astype(np.int64)
    keep = np.ones(len(k), dtype=bool)
    for p in homes:
        keep &= ((h - (int(p) % cap) + hole) % cap) >= 2 * hole
    assert int(keep.sum()) >= n
    return k[keep][:n]


def widen(k, seed=5):
    """64-bit keys -> 16-byte keys {w0 = k, w1}: the identity hash of a wide key is w0"""
    return np.stack([k, W.splitmix64(k + np.uint64(seed)) >> np.uint64(40)], axis=1)


def vals_for(n, base=0):
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(2**32)).astype(np.uint32) + np.uint32(base)


def shuffled(k, seed):
    return k[np.random.default_rng(seed).permutation(len(k))]


# ---- profile of a call, the refused call itself ---------------------------------------------------------------------------------
def profile_on(t):
    assert K.lib().kh_profile_enable(t._h, 1) == K.KH_OK          # (a wide handle is a kh_table: one profile for both key widths)
    assert K.lib().kh_profile_reset(t._h) == K.KH_OK


def profile_of(t):
    buf = C.create_string_buffer(1 << 16)
    assert K.lib().kh_profile_dump(t._h, buf, len(buf)) == K.KH_OK
    return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines()}


REFUSERS = ("k_build_fused", "k_insert_fused", "k_rebuild_fused", "k_chunk_place", "kw_chunk_place", "k_ip_apply", "k_ip_serial", "k_small_batch")


def refused(t, call, case):
    """runs `call`, which must be refused with KH_ERR_PROBE_OVERFLOW -> the profile of the refused call"""
    profile_on(t)
    with pytest.raises(kh.KhError) as ei:
        call()
    assert ei.value.status == K.KH_ERR_PROBE_OVERFLOW, ei.value
    assert "probe distance" in str(ei.value)
    p = profile_of(t)
    print("refused %s: %s" % (case, " ".join("%s=%d" % (k, p[k]) for k in REFUSERS if k in p)))
    return p


def usable_afterwards(g, o, kind=0, n=1000):
    """the next call succeeds and the table equals the oracle, which never saw the refused call"""
    fresh = spread(n, 9001, 1 << 12, [])
    fv = vals_for(len(fresh), 77)
    assert g.insert(dev(fresh), dev(fv)) == o.insert(fresh, fv) == len(fresh)
    check_state(g, o, kind)


# ---- the insert paths, one row each ------------------------------------------------------------------------------------------------------------
# cap0: capacity the table is created with; held: keys it holds; cap: capacity at which the batch is laid out (and refused);
# new / again / twice: records of the batch that are new keys, held keys, repeats of its own new keys; must: labels the refused call shows
ROWS = {
    "build_dups":     dict(cap0=128, held=0, cap=1 << 19, new=291_000, again=0, twice=9_000, must=("k_build_fused",)),
    "build_distinct": dict(cap0=128, held=0, cap=1 << 19, new=300_000, again=0, twice=0, must=("k_build_fused",)),
    "build_lean":     dict(cap0=1 << 23, held=0, cap=1 << 23, new=1_100_000, again=0, twice=0, must=("k_build_fused", "k_sample_dups")),
    "insert_z2":      dict(cap0=128, held=200_000, cap=1 << 19, new=180_000, again=15_000, twice=5_000, must=("k_insert_fused",)),
    "insert_stream":  dict(cap0=1 << 19, held=200_000, cap=1 << 19, new=45_000, again=10_000, twice=5_000, must=("k_insert_fused",)),
    "general":        dict(cap0=128, held=30_000, cap=1 << 17, new=30_000, again=30_000, twice=140_000, must=("k_dedup", "k_rebuild_fused")),
    "general_x4":     dict(cap0=128, held=30_000, cap=1 << 18, new=150_000, again=30_000, twice=20_000, must=("k_dedup", "k_chunk_place")),
}
LOADED = [r for r in ROWS if ROWS[r]["held"]]


def make_case(row, piles, held_piles=(), cls=RH, oracle=None):
    """-> (table holding the row's background + held_piles, its oracle, batch keys, batch values): the batch is the row's background
    records plus `piles` (lists of keys), shuffled"""
    R = ROWS[row]
    homes = [int(p[0]) & 0xFFFFFFFF for p in list(piles) + list(held_piles)]
    small = min(R["cap"], max(R["cap0"], 1 << 16))                   # no capacity the table passes through is smaller
    pool = spread(R["held"] + R["new"], 100 + len(row), small, homes)
    held, new = pool[:R["held"]], pool[R["held"]:R["held"] + R["new"]]
    kind = 0 if cls is RH else 1
    g = cls(R["cap0"], 0.35, 0.8, hash="identity")
    o = oracle.OracleTable(kind, R["cap0"], 0.35, 0.8, oracle.HASH_IDENTITY, 43)
    hk = np.concatenate([held] + list(held_piles))
    if len(hk):
        hv = vals_for(len(hk), 5)
        assert g.insert(dev(hk), dev(hv)) == o.insert(hk, hv) == len(hk)
    rng = np.random.default_rng(len(row))
    batch = np.concatenate([new, held[rng.integers(0, max(len(held), 1), R["again"])] if R["again"] else new[:0],
                            new[rng.integers(0, len(new), R["twice"])]] + list(piles))
    batch = shuffled(batch, 3)
    return g, o, batch, vals_for(len(batch), 1_000_000)


def accepted(g, o, batch, bv, R, kind=0):
    """the batch is taken: the oracle's count, the row's capacity, the oracle's layout and items -> the profile of the call (where each
    pile's last element stands is the caller's to check)"""
    profile_on(g)
    assert g.insert(dev(batch), dev(bv)) == o.insert(batch, bv)
    assert not o.probe_overflow()
    p = profile_of(g)
    assert g.capacity() == R["cap"]
    check_state(g, o, kind)
    return p


def lean_taken(p):
    return "k_sample_dups" in p and p.get("k_part_scatter") == 2 and "k_part_hist" not in p and "k_dedup" not in p and p.get("k_build_fused") == 1


MID = 5 * 2048 + 1000          # a home in the middle of chunk 5


# ---- the boundary, per path: 128 keys of one home bucket fit, 129 do not ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(ROWS))
def test_boundary_128_fit_129_do_not(oracle, row):
    R = ROWS[row]
    g, o, batch, bv = make_case(row, [pile(MID, 128)], oracle=oracle)
    p = accepted(g, o, batch, bv, R)
    assert g.export_info()[MID + 127] == 0xFF and int(np.flatnonzero(g.displacement_histogram())[-1]) == 127
    assert all(lbl in p for lbl in R["must"] if lbl not in ("k_dedup", "k_rebuild_fused", "k_chunk_place")), p
    if row == "build_lean":
        assert lean_taken(p), p
    elif row.startswith(("build", "insert")):
        assert "k_dedup" not in p, p                                  # the one-launch form was taken and accepted
    g.close(); o.close()
    g, o, batch, bv = make_case(row, [pile(MID, 129)], oracle=oracle)
    snap = snapshot(g)
    p = refused(g, lambda: g.insert(dev(batch), dev(bv)), row + " 129")
    assert all(lbl in p for lbl in R["must"]), p
    assert_unchanged(g, snap, pile(MID, 129))
    usable_afterwards(g, o)
    g.close(); o.close()


@pytest.mark.parametrize("row", LOADED)
def test_boundary_split_between_table_and_batch(oracle, row):
    """100 of the pile in the table, 29 in the batch: the overflow exists only in old and new elements together; 28 are taken"""
    R = ROWS[row]
    pk = pile(MID, 129)
    g, o, batch, bv = make_case(row, [pk[100:128]], [pk[:100]], oracle=oracle)
    accepted(g, o, batch, bv, R)
    assert g.export_info()[MID + 127] == 0xFF
    g.close(); o.close()
    g, o, batch, bv = make_case(row, [pk[100:]], [pk[:100]], oracle=oracle)
    snap = snapshot(g)
    p = refused(g, lambda: g.insert(dev(batch), dev(bv)), row + " 100+29")
    assert all(lbl in p for lbl in R["must"]), p
    assert_unchanged(g, snap, pk[100:])
    usable_afterwards(g, o)
    g.close(); o.close()


@pytest.mark.parametrize("split", [False, True])
def test_wide_general_path_boundary(split):
    """the wide table has the general path alone (kw_dedup + kw_chunk_place): 30 000 held + 60 000 records, the capacity doubles; against
    oracle/wide_model.py.  split: 100 of the pile are in the table already"""
    from oracle.wide_model import WideModel
    pool = spread(60_000, 111, 1 << 16, [MID])
    held, new, pk = pool[:30_000], pool[30_000:], pile(MID, 129)
    hp = pk[:100] if split else pk[:0]
    rng = np.random.default_rng(112)
    for m in (128, 129):
        g = WIDE(128, 0.35, 0.8, hash="identity"); mod = WideModel(128, 0.35, 0.8, "identity", 43)
        hk = widen(np.concatenate([held, hp])); hv = vals_for(len(hk), 5)
        assert g.insert(dev(hk), dev(hv)) == mod.insert(hk, hv) == len(hk)
        bk = widen(shuffled(np.concatenate([new, held[rng.integers(0, 30_000, 20_000)], new[rng.integers(0, 30_000, 10_000)], pk[len(hp):m]]), 3))
        bv = vals_for(len(bk), 1_000_000)
        if m == 129:
            snap = snapshot(g)
            p = refused(g, lambda: g.insert(dev(bk), dev(bv)), "wide general%s" % (" 100+29" if split else " 129"))
            assert "kw_dedup" in p and "kw_chunk_place" in p, p
            assert_unchanged(g, snap, widen(pk[len(hp):m]))
            assert mod.insert(bk, bv) is None and mod.probe_overflow
            bk = widen(spread(1000, 9001, 1 << 12, [])); bv = vals_for(1000, 77)          # the next call is taken
        assert g.insert(dev(bk), dev(bv)) == mod.insert(bk, bv)
        assert (g.size(), g.capacity()) == (mod.size(), mod.capacity())
        assert np.array_equal(g.export_info(), mod.export_info())
        for a, b in zip(g.sorted_items(), mod.sorted_items()):
            assert np.array_equal(a, b)
        if m == 128:
            assert g.capacity() == 1 << 17 and g.export_info()[MID + 127] == 0xFF
        g.close(); mod.close()


def test_rehash_to_twice_the_capacity_keeps_a_full_pile(oracle):
    """k_rebuild_fused lays a 128-pile out again at the doubled capacity (a larger capacity never merges home buckets: no refusal here)"""
    g, o, batch, bv = make_case("insert_z2", [pile(MID, 128)], oracle=oracle)
    accepted(g, o, batch, bv, ROWS["insert_z2"])
    profile_on(g)
    g.rehash(2 * g.capacity()); o.rehash(2 * o.capacity())
    assert "k_rebuild_fused" in profile_of(g)
    check_state(g, o, 0)
    assert g.export_info()[MID + 127] == 0xFF
    g.close(); o.close()


# ---- where the pile lies: across a chunk boundary, across the end of the table, pushed by the chunk before ------------------------------------------------------------------------------------------------------
def place(where, cap):
    return 2048 * 7 - 60 if where == "straddle" else cap - 60


@pytest.mark.parametrize("row", ["build_lean", "insert_stream", "general"])
@pytest.mark.parametrize("where", ["straddle", "wrap"])
def test_pile_across_a_chunk_boundary_and_across_the_end(oracle, row, where):
    """a pile at 2048 c - 60 runs over into the next chunk, one at cap - 60 into slot 0: 120 fit, 140 do not"""
    R = ROWS[row]
    home = place(where, R["cap"])
    g, o, batch, bv = make_case(row, [pile(home, 120)], oracle=oracle)
    p = accepted(g, o, batch, bv, R)
    assert g.export_info()[(home + 119) % R["cap"]] == 0x80 | 119
    if row == "build_lean":
        assert lean_taken(p), p
    g.close(); o.close()
    g, o, batch, bv = make_case(row, [pile(home, 140)], oracle=oracle)
    snap = snapshot(g)
    p = refused(g, lambda: g.insert(dev(batch), dev(bv)), "%s %s 140" % (row, where))
    assert all(lbl in p for lbl in R["must"]), p
    assert_unchanged(g, snap, pile(home, 140))
    usable_afterwards(g, o)
    g.close(); o.close()


@pytest.mark.parametrize("row", ["build_lean", "insert_stream", "general"])
def test_overflow_that_exists_only_through_the_carry_in(oracle, row):
    """100 keys at 2048 c - 50 and 100 at 2048 c + 5: each pile fits alone, the first pushes the second to distance 100 + 100 - 55 - 1 = 144
    -- inside chunk c that is visible only through the run-over of chunk c - 1.  With 80 in the first the largest distance is 124."""
    R = ROWS[row]
    a, b = 2048 * 7 - 50, 2048 * 7 + 5
    g, o, batch, bv = make_case(row, [pile(a, 80), pile(b, 100)], oracle=oracle)
    assert not canonical_info(np.concatenate([pile(a, 80), pile(b, 100)]) & np.uint64(R["cap"] - 1), R["cap"])[1]
    p = accepted(g, o, batch, bv, R)
    assert int(np.flatnonzero(g.displacement_histogram())[-1]) == 124 and g.export_info()[b + 124] == 0x80 | 124
    assert_consistent(g)
    if row == "build_lean":
        assert lean_taken(p), p
    g.close(); o.close()
    g, o, batch, bv = make_case(row, [pile(a, 100), pile(b, 100)], oracle=oracle)
    assert canonical_info(np.concatenate([pile(a, 100), pile(b, 100)]) & np.uint64(R["cap"] - 1), R["cap"])[1]
    snap = snapshot(g)
    p = refused(g, lambda: g.insert(dev(batch), dev(bv)), row + " carry-in")
    assert all(lbl in p for lbl in R["must"]), p
    assert_unchanged(g, snap, np.concatenate([pile(a, 100), pile(b, 100)]))
    usable_afterwards(g, o)
    g.close(); o.close()


# ---- reducer inserts are rolled back --------------------------------------------------------------------------------------------------------
OPS4 = ["plus", "min", "max", "or"]


def reducer_case(wide, cls=None):
    """a table of 30 000 keys and a twin; a batch that names 10 000 of them (2 000 twice), 20 000 new spread keys and a 129-pile"""
    cls = cls or (WIDE if wide else RH)
    pool = spread(54_000, 61, 1 << 16, [MID])
    held, new, pk = pool[:30_000], pool[30_000:50_000], pile(MID, 129)
    bk = shuffled(np.concatenate([held[:10_000], held[:2_000], new, pk]), 62)
    if wide:
        held, new, pk, bk = widen(held), widen(new), widen(pk), widen(bk)
    hv, bv = draw_vals(len(held), 63), draw_vals(len(bk), 64)
    g, twin = cls(128, 0.35, 0.8, hash="identity"), cls(128, 0.35, 0.8, hash="identity")
    assert g.insert(dev(held), dev(hv)) == twin.insert(dev(held), dev(hv)) == 30_000
    return g, twin, held, hv, new, pk, bk, bv


def changes_stored_values(g, bk, bv, op):
    """the batch without its pile changes thousands of stored values under `op` (else the roll-back would have nothing to restore)"""
    before = g.sorted_items()
    w0 = bk if bk.ndim == 1 else bk[:, 0]
    keep = (w0 & np.uint64(0xFFFFFFFF)) != np.uint64(MID)
    ek, ev = combined(before, bk[keep], bv[keep], op)
    if ek.ndim == 1:
        was_held = np.isin(ek, before[0])
    else:
        hs = set(map(tuple, before[0].tolist()))
        was_held = np.array([tuple(r) in hs for r in ek.tolist()])
    assert int(was_held.sum()) == len(before[1]) and int((ev[was_held] != before[1]).sum()) > 1000


@pytest.mark.parametrize("op", OPS4)
@pytest.mark.parametrize("table", ["rh_immediate", "rh_deferred", "wide"])
def test_reducer_insert_is_rolled_back(monkeypatch, table, op):
    """min / max / or cannot be undone from their result: the apply step saves the value each slot held (k_dedup where it applies at once,
    k_apply_reduce(+1) with KH_DISABLE_PLUS_IMMEDIATE) and the refused re-layout stores it back.  Values included: the point of the case.
    The 64-bit table runs both saves, the wide table has the k(w)_apply_reduce(+1) save alone.
    Limitation: nothing observable says which save ran.  rh_immediate takes the save inside k_dedup only while the host finds the
    partition offsets exact (32 129 records, 2^6 partitions: no histogram-free partition below 2^12) and k_dedup folds each partition in
    one class (about 500 records per partition against a staging area of 2048); the apply kernel is launched in both cases (it skips
    the partitions k_dedup applied itself), so the profile labels are the same.  Should this shape stop meeting those two conditions,
    both cases would run the k_apply_reduce(+1) save and no assertion here would notice."""
    if table == "rh_deferred":
        monkeypatch.setenv("KH_DISABLE_PLUS_IMMEDIATE", "1")          # read with getenv at every call
    g, twin, held, hv, new, pk, bk, bv = reducer_case(table == "wide")
    changes_stored_values(g, bk, bv, op)
    snap = snapshot(g)
    p = refused(g, lambda: g.insert_reduce(dev(bk), dev(bv), op), "%s reduce %s" % (table, op))
    apply = ("kw_apply_plus" if op == "plus" else "kw_apply_reduce") if table == "wide" else ("k_apply_plus" if op == "plus" else "k_apply_reduce")
    assert apply in p and ("kw_dedup" if table == "wide" else "k_dedup") in p, p
    assert_unchanged(g, snap, np.concatenate([new, pk]))
    # the same batch without the last pile key is taken, by the table and by its twin that never saw the refused call
    last = (bk if bk.ndim == 1 else bk[:, 0]) == (pk if pk.ndim == 1 else pk[:, 0])[-1]
    assert g.insert_reduce(dev(bk[~last]), dev(bv[~last]), op) == twin.insert_reduce(dev(bk[~last]), dev(bv[~last]), op) == 20_128
    for a, b in zip(g.sorted_items(), twin.sorted_items()):
        assert np.array_equal(a, b)
    assert np.array_equal(g.export_info(), twin.export_info()) and g.capacity() == twin.capacity()
    assert_consistent(g)
    g.close(); twin.close()


@pytest.mark.parametrize("op", OPS4)
@pytest.mark.parametrize("wide", [False, True])
def test_streamed_reducer_insert_is_rolled_back(wide, op):
    """insert_begin(reduce=op), three feeds, insert_end refused: table unchanged, no streamed insert left open"""
    g, twin, held, hv, new, pk, bk, bv = reducer_case(wide, WIDE_STREAM if wide else None)
    twin.close()
    snap = snapshot(g)
    cuts = [0, 11_000, 11_001, len(bk)]
    dk, dv = dev(bk), dev(bv)

    def streamed():
        g.insert_begin(len(bk), reduce=op)
        for a, b in zip(cuts[:-1], cuts[1:]):
            g.insert_feed(dk[a:b], dv[a:b])
        g.insert_end()
    refused(g, streamed, "%s streamed reduce %s" % ("wide" if wide else "rh", op))
    assert_unchanged(g, snap, np.concatenate([new, pk]))          # (any query is refused while a streamed insert is open)
    g.insert_begin(2, reduce=op)                                    # a new streamed insert is accepted
    g.insert_feed(dev(new[:2]), dev(bv[:2]))
    assert g.insert_end() == 2 and g.size() == snap["size"] + 2
    assert_consistent(g)
    g.close()


def test_update_is_refused_before_it_assigns():
    """update() with the same batch: the re-layout is refused before k_dedup_assign runs, old values stay"""
    g, twin, held, hv, new, pk, bk, bv = reducer_case(False)
    twin.close()
    snap = snapshot(g)
    p = refused(g, lambda: g.update(dev(bk), dev(bv)), "update")
    assert "k_dedup_assign" not in p, p
    assert_unchanged(g, snap, np.concatenate([new, pk]))
    g.close()


@pytest.mark.parametrize("row", ["build_dups", "insert_z2", "general"])
@pytest.mark.parametrize("m", [129, 300])
def test_linear_probe_has_no_distance_limit(oracle, row, m):
    """control: the same batches into the linear-probe table, whose fused kernels keep the same 5-bit distance code in LDS"""
    g, o, batch, bv = make_case(row, [pile(MID, m)], cls=LP, oracle=oracle)
    profile_on(g)
    assert g.insert(dev(batch), dev(bv)) == o.insert(batch, bv)
    p = profile_of(g)
    assert all(lbl in p for lbl in ROWS[row]["must"] if lbl != "k_rebuild_fused"), p
    check_state(g, o, 1)
    assert host_count(g, pile(MID, m)).all()
    g.close(); o.close()


# ---- re-layouts that merge home buckets ---------------------------------------------------------------------------------------
def test_rehash_to_a_smaller_capacity_that_merges_homes(oracle):
    """the 130 keys 5 + 1024 j: sixteen buckets among 16384 (eight or nine keys each), one bucket among 1024, two among 2048"""
    merge = np.uint64(5) + np.arange(130, dtype=np.uint64) * np.uint64(1024)
    keys = np.concatenate([spread(200, 71, 1024, [], 0), merge])
    vals = vals_for(len(keys))
    g = RH(16384, 0.35, 0.8, hash="identity"); o = oracle.OracleTable(0, 16384, 0.35, 0.8, oracle.HASH_IDENTITY, 43)
    assert g.insert(keys, vals) == o.insert(keys, vals) == len(keys)
    snap = snapshot(g)
    p = refused(g, lambda: g.rehash(1024), "rehash(1024)")
    assert "k_chunk_place" in p, p
    assert_unchanged(g, snap)
    assert g.insert(merge[:3], vals[:3]) == 0                       # the table takes the next call
    assert_unchanged(g, snap)
    g.rehash(2048); o.rehash(2048)                                  # 65 keys on each of the buckets 5 and 1029
    assert g.capacity() == 2048 and not o.probe_overflow()
    check_state(g, o, 0)
    usable_afterwards(g, o, n=100)
    g.close(); o.close()


def test_erase_one_whose_halving_cannot_be_laid_out(oracle):
    """capacity 1024, 65 keys on each of the homes 5 and 517, below min_load: erase_one erases, then asks for 512 buckets, where the
    130 share bucket 5.  Pinned (and said in the header at kh_erase_one): the key is gone, the status is KH_ERR_PROBE_OVERFLOW, the
    capacity stays; the table is consistent and goes on working."""
    merge = np.uint64(5) + np.arange(130, dtype=np.uint64) * np.uint64(512)
    bg = spread(200, 72, 512, [], 0)
    keys = np.concatenate([bg, merge])
    vals = vals_for(len(keys))
    g = RH(1024, 0.35, 0.8, hash="identity"); o = oracle.OracleTable(0, 1024, 0.35, 0.8, oracle.HASH_IDENTITY, 43)
    assert g.insert(keys, vals) == o.insert(keys, vals) == len(keys)
    assert g.capacity() == 1024 and g.size() < g.load_thresholds()[0]
    p = refused(g, lambda: g.erase_one(int(bg[0])), "erase_one")
    assert "k_chunk_place" in p, p
    assert g.capacity() == 1024 and g.size() == len(keys) - 1 and not host_count(g, bg[:1]).any()
    assert_consistent(g)
    # the oracle for the same state: the erase in a table that cannot shrink
    o.set_min_load_factor(0.0)
    assert o.erase_one(int(bg[0])) == 1
    o.set_min_load_factor(0.35)
    check_state(g, o, 0)
    g.set_min_load_factor(0.0); o.set_min_load_factor(0.0)
    assert g.erase_one(int(merge[7])) == o.erase_one(int(merge[7])) == 1
    check_state(g, o, 0)
    g.close(); o.close()


# ---- batches applied in place: mid-size and small -------------------------------------------------------------------------------------------------
def test_in_place_batch_applies_what_fits(oracle):
    """capacity 2^20, 5e5 held, 1 500 records with a 129-pile: applied in place, key by key.  Each key is either inserted whole or left
    out, and a key is left out only if its own insertion would push an element to distance 128: here exactly one pile key.  Every
    other key of the batch is applied; the status is KH_ERR_PROBE_OVERFLOW and its text says that the keys that fit were applied."""
    cap = 1 << 20
    pool = spread(502_000, 81, cap, [MID])
    held, new, pk = pool[:500_000], pool[500_000:501_000], pile(MID, 129)
    hv = vals_for(len(held), 9)
    for m in (128, 129):
        g = RH(cap, 0.35, 0.8, hash="identity"); o = oracle.OracleTable(0, cap, 0.35, 0.8, oracle.HASH_IDENTITY, 43)
        assert g.insert(dev(held), dev(hv)) == o.insert(held, hv) == len(held)
        bk = shuffled(np.concatenate([new, held[:300], new[:71], pk[:m]]), 82)
        bv = vals_for(len(bk), 500)
        before = snapshot(g)
        profile_on(g)
        if m == 128:
            assert g.insert(dev(bk), dev(bv)) == o.insert(bk, bv) == 1128
            p = profile_of(g)
            assert g.export_info()[MID + 127] == 0xFF
            check_state(g, o, 0)
        else:
            with pytest.raises(kh.KhError) as ei:
                g.insert(dev(bk), dev(bv))
            assert ei.value.status == K.KH_ERR_PROBE_OVERFLOW and "applied in place" in str(ei.value)
            p = profile_of(g)
            print("refused in place: " + " ".join("%s=%d" % (k, p[k]) for k in REFUSERS if k in p))
            assert_consistent(g)
            k, v = g.sorted_items()
            assert g.capacity() == cap and thresholds(g) == before["thresholds"]
            assert np.isin(before["keys"], k).all() and np.isin(k, np.concatenate([before["keys"], bk])).all()
            assert int(np.isin(pk, k).sum()) == 128 and np.isin(new, k).all() and g.size() == 500_000 + 1000 + 128
            old = np.isin(k, before["keys"])
            assert np.array_equal(v[old], before["vals"])                      # plain insert: old keys keep their values
            first = {}
            for kk, vv in zip(bk.tolist(), bv.tolist()):
                first.setdefault(kk, vv)
            assert np.array_equal(v[~old], np.array([first[kk] for kk in k[~old].tolist()], dtype=np.uint32))      # first value wins
            # the table goes on working: the oracle given exactly the keys that were applied
            ok = k[~old]
            o.insert(ok, v[~old])
            usable_afterwards(g, o)
        assert "k_ip_apply" in p and "k_ip_serial" in p and "k_chunk_place" not in p and "k_rebuild_fused" not in p and "k_insert_fused" not in p, p
        g.close(); o.close()


@pytest.mark.parametrize("mode", ["insert", "update", "plus", "max"])
def test_small_batch_applies_the_keys_before_the_first_that_does_not_fit(mode):
    """<= 16 keys go one by one through k_small_batch, which stops at the first key whose insertion would push an element to distance
    128; that key AND the rest of the batch go to the general path, whose re-layout is refused as a whole.  127 of a pile held; the
    batch [fresh A, held H1, pile key 128, pile key 129, fresh B, held H2]: A, H1's update / reduction and the 128th are applied, the
    129th is not, and neither are B and H2 although they would fit."""
    home = 4000
    bg = spread(300, 131, 1 << 14, [home])
    pk = pile(home, 129)
    hk = np.concatenate([bg[:298], pk[:127]]); hv = draw_vals(len(hk), 132)
    hv[10], hv[20] = 5, 7                                            # H1, H2: every mode but insert changes 5
    g = RH(1 << 14, 0.35, 0.8, hash="identity")
    assert g.insert(hk, hv) == len(hk)
    A, B, H1, H2 = bg[298], bg[299], bg[10], bg[20]
    bk = np.array([A, H1, pk[127], pk[128], B, H2], dtype=np.uint64)
    bv = np.array([11, 0xFFFFFFF0, 13, 14, 15, 0xFFFFFFF1], dtype=np.uint32)
    before = dict(zip(*[x.tolist() for x in g.sorted_items()]))
    call = {"insert": lambda: g.insert(bk, bv), "update": lambda: g.update(bk, bv)}.get(mode, lambda: g.insert_reduce(bk, bv, mode))
    p = refused(g, call, "small batch " + mode)
    assert "k_small_batch" in p and ("k_rebuild_fused" in p or "k_chunk_place" in p) and "k_dedup_assign" not in p, p
    after = dict(zip(*[x.tolist() for x in g.sorted_items()]))
    exp = dict(before)
    exp[int(A)] = 11; exp[int(pk[127])] = 13
    h1 = before[int(H1)]
    exp[int(H1)] = {"insert": h1, "update": 0xFFFFFFF0, "plus": (h1 + 0xFFFFFFF0) & 0xFFFFFFFF, "max": max(h1, 0xFFFFFFF0)}[mode]
    assert exp[int(H1)] != h1 or mode == "insert"
    assert after == exp                                             # B and the 129th absent, H2 as it was
    assert g.size() == len(hk) + 2 and g.capacity() == 1 << 14
    assert_consistent(g)
    assert g.export_info()[home + 127] == 0xFF
    assert g.insert(bk[4:5], bv[4:5]) == 1 and g.size() == len(hk) + 3          # the table goes on working: B alone fits
    assert_consistent(g)
    g.close()


# ---- the position index ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_failed_append_and_failed_build_leave_the_index_empty(wide):
    cls = kh.WideKmerPositionIndex if wide else kh.KmerPositionIndex
    mk = (lambda: cls(k=63, hash="identity")) if wide else (lambda: cls(k=31, hash="identity"))
    w = widen if wide else (lambda a: a)
    good = spread(20_000, 91, 1 << 15, [MID])
    gk = w(np.concatenate([good, good[:3000]]))                    # some k-mers occur twice
    gp = np.arange(len(gk), dtype=np.uint32)
    bad = w(shuffled(np.concatenate([spread(5000, 92, 1 << 15, [MID]), good[:500], pile(MID, 129)]), 93))
    bp = np.arange(len(bad), dtype=np.uint32) + np.uint32(1 << 20)
    fresh = mk()
    cap_fresh = fresh.capacity()
    fresh.build(dev(gk), dev(gp))
    want = fresh.export()
    x = mk()
    for how in ("append", "build"):
        if how == "append":
            x.build(dev(gk), dev(gp))
            assert x.size() == 20_000 and x.total() == len(gk)
        with pytest.raises(kh.KhError) as ei:
            (x.append if how == "append" else x.build)(dev(bad), dev(bp))
        assert ei.value.status == K.KH_ERR_PROBE_OVERFLOW and "probe distance" in str(ei.value), (how, ei.value)      # the table's own text
        assert x.size() == x.total() == 0 and x.capacity() == cap_fresh, how
        ek, eo, ep = x.export()
        assert len(ek) == 0 and len(ep) == 0 and eo.tolist() == [0]
        assert not np.asarray(x.count(gk)).any()
        x.build(dev(gk), dev(gp))                                    # the same handle builds again: byte for byte a fresh index
        for a, b in zip(x.export(), want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert x.capacity() == fresh.capacity()
        x.clear()
    x.close(); fresh.close()
