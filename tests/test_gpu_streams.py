"""GPU: stream ordering of every entry point that takes device memory, against the CPU references of the suite.

The other GPU tests run on the null stream, where a call issued on the wrong stream still computes the right answer.  Here every
device input is a stream_checks.late_input: it holds a well-formed DECOY until a delay on the caller's side stream has run and the
real data only afterwards, and assert_busy() right before the call under test shows that the delay was still running when the call
was made.  A call that runs on another stream, or a handle that loses order when its stream changes, therefore computes a wrong
answer from valid memory -- a value mismatch against the oracle, never a fault.

    A  late input on the caller's side stream: tables, indexes, front ends, HyperLogLog
    B  one object, two streams: calls on one handle take effect in call order, whichever streams they were issued under
    C  two objects: a call that reads a second handle is ordered after that handle's pending work
    D  the sharded table's exchange pipeline under a caller's side stream (one rank over RCCL, forced collectives, a child process)

Every mutating call of a table or an index returns a count and so has drained its stream when it returns; the calls that leave work
pending are count / find_values(want_total=False) with device queries, insert_feed, hash_batch and the HyperLogLog updates, merge and
clear.  Group B therefore switches streams behind those, and also checks that a handle keeps its state over a plain switch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402
from kmerhash_amd import wide as KW  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402
from kmerhash_amd.hll import hyperloglog64  # noqa: E402
from kmerhash_amd.index import KmerPositionIndex, WideKmerPositionIndex  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle.kmers_np import np_kmers, np_kmers_fastq  # noqa: E402
from oracle.wide_model import WideModel  # noqa: E402
from index_model import IndexModel, np_kmers_fastq_pos, np_kmers_pos, np_window_positions  # noqa: E402
from minimizer_model import np_minimizers  # noqa: E402
from stream_checks import assert_busy, consume_on, late_input, late_inputs, side_stream, to_dev  # noqa: E402
from syncmer_model import np_is_syncmer, np_kmers128, np_syncmers  # noqa: E402
from wide_index_model import WideIndexModel  # noqa: E402

M32 = 0xFFFFFFFF
MURMUR = O.HASH_MURMUR3_X64          # the order hash "murmur" of the samplers
REDUCE = {"plus": lambda a, b: (a + b) & M32, "min": min, "max": max, "or": lambda a, b: a | b}


@pytest.fixture()
def s():
    st = side_stream()
    yield st
    st.synchronize()


@pytest.fixture()
def s1():
    st = side_stream()
    yield st
    st.synchronize()


@pytest.fixture()
def s2(s1):
    st = side_stream(s1)
    yield st
    st.synchronize()


def rehearse(stream, call):
    """the call under test once before, under the same stream, on decoys and (where it changes its object) on a twin object, so that
    the device allocations of the real call -- torch's per-stream cache for the outputs, the library's pool -- are served from memory at
    hand: a first allocation from the driver can take longer than a delay lasts, and a call that spent the delay allocating would read
    its late input in order whatever stream it ran on."""
    with torch.cuda.stream(stream):
        call()
    torch.cuda.synchronize()


def u64(t):
    return np.ascontiguousarray(t).view(np.uint64)


def u32(t):
    return np.ascontiguousarray(t).view(np.uint32)


# ---- data: real inputs and decoys of the same shape and kind ----------------------------------------------------------------------
def wide_rows(n, seed):
    """n distinct 16-byte keys (n, 2)"""
    return np.ascontiguousarray(np.stack([W.distinct_u64(n, seed=seed), W.distinct_u64(n, seed=seed + 1000)], axis=1))


def random_text(n, seed, n_bad=3):
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    if n_bad:
        t[rng.integers(0, n, n_bad)] = ord("N")
    return t


TEXT_N = 12_000          # three tiles of 4096 start positions, ragged
TEXT = random_text(TEXT_N, 1)
TEXT_DECOY = random_text(TEXT_N, 2, n_bad=0)
FASTQ = np.frombuffer(KM.synthetic_fastq(60, 100, 5000, seed=3), dtype=np.uint8).copy()
FASTQ_DECOY = np.frombuffer(KM.synthetic_fastq(60, 100, 5000, seed=4), dtype=np.uint8).copy()
assert FASTQ.shape == FASTQ_DECOY.shape and not np.array_equal(FASTQ, FASTQ_DECOY)


class Narrow:
    """a 64-bit-key table next to its oracle, pre-filled through host arrays (no stream is involved)"""
    wide = False
    CAP, NBASE = 1 << 16, 20_000          # 128 regions of 512 slots: 17..128 keys go in place, <= 16 by one lane

    def __init__(self, kind, prefill=True):
        self.kind = kind
        cls = kh.hashmap_robinhood_doubling if kind == 0 else kh.hashmap_linearprobe_doubling
        self.g = cls(self.CAP, 0.35, 0.8)
        self.o = O.OracleTable(kind, self.CAP, 0.35, 0.8)
        self.base = W.distinct_u64(self.NBASE, seed=101)
        if prefill:
            bv = np.arange(self.NBASE, dtype=np.uint32) + np.uint32(5)
            assert self.g.insert(self.base, bv) == self.o.insert(self.base, bv)

    def fresh(self, n, seed):
        return W.distinct_u64(n, seed=seed)

    def items(self):
        k, v = self.o.sorted_items()
        return dict(zip(k.tolist(), v.tolist()))

    @staticmethod
    def rows(keys):
        return np.asarray(keys, dtype=np.uint64).tolist()

    @staticmethod
    def sorted_arrays(d):
        ks = sorted(d)
        return np.array(ks, dtype=np.uint64), np.array([d[k] for k in ks], dtype=np.uint32)

    def check(self):
        assert (self.g.size(), self.g.capacity()) == (self.o.size(), self.o.capacity())
        for a, b in zip(self.g.sorted_items(), self.o.sorted_items()):
            assert np.array_equal(a, b)

    def close(self):
        self.g.close()


class Wide:
    """the 16-byte-key table next to its model"""
    wide = True
    CAP, NBASE = 1 << 14, 5_000

    def __init__(self, kind=0, prefill=True):
        self.g = KW.hashmap_robinhood_doubling_wide_stream(self.CAP, 0.4, 0.9)
        self.o = WideModel(self.CAP, 0.4, 0.9)
        self.base = wide_rows(self.NBASE, 101)
        if prefill:
            bv = np.arange(self.NBASE, dtype=np.uint32) + np.uint32(5)
            assert self.g.insert(self.base, bv) == self.o.insert(self.base, bv)

    def fresh(self, n, seed):
        return wide_rows(n, seed)

    def items(self):
        k, v = self.o.sorted_items()
        return dict(zip(map(tuple, k.tolist()), v.tolist()))

    @staticmethod
    def rows(keys):
        return list(map(tuple, np.asarray(keys, dtype=np.uint64).reshape(-1, 2).tolist()))

    @staticmethod
    def sorted_arrays(d):
        ks = sorted(d, key=lambda k: (k[1], k[0]))
        return np.array(ks, dtype=np.uint64).reshape(-1, 2), np.array([d[k] for k in ks], dtype=np.uint32)

    def check(self):
        assert (self.g.size(), self.g.capacity()) == (self.o.size(), self.o.capacity())
        for a, b in zip(self.g.sorted_items(), self.o.sorted_items()):
            assert np.array_equal(a, b)

    def close(self):
        self.g.close(); self.o.close()


TABLES = [("rh", Narrow, 0), ("lp", Narrow, 1), ("wide", Wide, 0)]
SIZES = {"rh": (8, 100, 100_000), "lp": (8, 100, 100_000), "wide": (8, 50_000)}
TABLE_SIZES = [(name, cls, kind, n) for name, cls, kind in TABLES for n in SIZES[name]]
IDS = ["%s-%d" % (t[0], t[3]) for t in TABLE_SIZES]


def batch(T, n, seed):
    """real (keys, vals): half new keys, a quarter keys the table holds, the rest repeats of the new ones, shuffled; and a decoy of
    n other new keys with other values"""
    rng = np.random.default_rng(seed)
    new = T.fresh(n, seed + 1)
    k = np.concatenate([new[: n - n // 2], T.base[rng.integers(0, len(T.base), n // 4)], new[: n // 2 - n // 4]])[rng.permutation(n)]
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dk = T.fresh(n, seed + 2)
    dv = (v ^ np.uint32(0x5A5A5A5A)).astype(np.uint32)
    return np.ascontiguousarray(k), v, dk, dv


def queries(T, n, seed):
    """real: hits and misses alternating; decoy: the same with hits and misses swapped"""
    rng = np.random.default_rng(seed)
    hit, miss = T.base[rng.integers(0, len(T.base), n)], T.fresh(n, seed + 7)
    sel = (np.arange(n) % 2 == 0)
    sel = sel if not T.wide else sel[:, None]
    return np.ascontiguousarray(np.where(sel, hit, miss)), np.ascontiguousarray(np.where(sel, miss, hit))


# ---- A. late input on the caller's side stream: tables ----------------------------------------------------------------------------
MUTATIONS = [t + (op,) for t in TABLE_SIZES for op in ("insert", "plus", "other", "update") if not (t[1] is Wide and op == "update")]


@pytest.mark.parametrize("name,cls,kind,n,op", MUTATIONS, ids=["%s-%d-%s" % (t[0], t[3], t[4]) for t in MUTATIONS])
def test_a_table_mutations(s, name, cls, kind, n, op):
    """insert, insert_reduce ("plus" and one more: "max" on the Robin Hood tables, "min" on linear probing), update (64-bit tables)"""
    T = cls(kind)
    k, v, dk, dv = batch(T, n, 11)
    before = T.items()
    other = "max" if kind == 0 else "min"
    twin = cls(kind)
    rop = "plus" if op == "plus" else other
    rehearse(s, lambda: (twin.g.insert if op == "insert" else twin.g.update)(to_dev(dk), to_dev(dv)) if op in ("insert", "update")
             else twin.g.insert_reduce(to_dev(dk), to_dev(dv), rop))
    twin.close()
    with torch.cuda.stream(s):
        bk, bv = late_inputs(s, (k, dk), (v, dv))
        assert_busy(s)
        if op == "insert":
            got = T.g.insert(bk, bv)
        elif op == "update":
            got = T.g.update(bk, bv)
        else:
            got = T.g.insert_reduce(bk, bv, rop)
    if op == "insert":
        assert got == T.o.insert(k, v)
        T.check()
    else:
        f = (lambda a, b: b) if op == "update" else REDUCE[rop]
        exp = dict(before)
        for kk, vv in zip(T.rows(k), v.tolist()):
            exp[kk] = f(exp[kk], vv) if kk in exp else vv
        assert T.g.size() == len(exp)
        if op != "update":
            assert got == len(exp) - len(before)
        for a, b in zip(T.g.sorted_items(), T.sorted_arrays(exp)):
            assert np.array_equal(a, b)
    T.close()


@pytest.mark.parametrize("op", ["count", "find_values", "find", "erase"])
@pytest.mark.parametrize("name,cls,kind,n", TABLE_SIZES, ids=IDS)
def test_a_table_queries_and_erase(s, name, cls, kind, n, op):
    T = cls(kind)
    q, dq = queries(T, n, 13)
    twin = cls(kind)
    rehearse(s, lambda: getattr(twin.g if op == "erase" else T.g, op)(to_dev(dq)))
    twin.close()
    with torch.cuda.stream(s):
        bq = late_input(s, q, dq)
        assert_busy(s)
        if op == "count":
            got = consume_on(s, T.g.count(bq))
            assert np.array_equal(got, T.o.count(q))
        elif op == "find_values":
            vals, found = consume_on(s, *T.g.find_values(bq))
            ev, ef = T.o.find(q) if cls is Narrow else T.o.find_values(q)
            assert np.array_equal(found, ef) and np.array_equal(u32(vals)[ef == 1], ev[ef == 1]) and not u32(vals)[ef == 0].any()
        elif op == "find":
            fk, fv = consume_on(s, *T.g.find(bq))
            ek, ev = T.o.find_compact(q) if cls is Narrow else T.o.find(q)
            assert np.array_equal(u64(fk), ek) and np.array_equal(u32(fv), ev)
        else:
            assert T.g.erase(bq) == T.o.erase(q)
            T.check()
    T.close()


@pytest.mark.parametrize("name,cls,kind", TABLES, ids=[t[0] for t in TABLES])
def test_a_streamed_insert_every_piece_late(s, name, cls, kind):
    T = cls(kind, prefill=False)
    k, v, dk, dv = batch(T, 40_000, 17)
    cuts = [0, 15_000, 15_000 + 4097, 40_000]
    twin = cls(kind, prefill=False)

    def feed_decoys():
        twin.g.insert_begin(40_000)
        held = [(to_dev(dk[a:b]), to_dev(dv[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
        for piece in held:
            twin.g.insert_feed(*piece)
        twin.g.insert_end()
    rehearse(s, feed_decoys)
    twin.close()
    with torch.cuda.stream(s):
        T.g.insert_begin(40_000)
        pieces = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            pieces.append(late_inputs(s, (k[a:b], dk[a:b]), (v[a:b], dv[a:b])))
            assert_busy(s)
            T.g.insert_feed(*pieces[-1])
        assert T.g.insert_end() == T.o.insert(k, v)
    T.check()
    T.close()


@pytest.mark.parametrize("name,cls,kind", TABLES, ids=[t[0] for t in TABLES])
def test_a_select_values_and_merge_across_streams(s1, s2, name, cls, kind):
    """`other` is filled under s1, `self` under s2; select_values(device=True) and merge run under s2 and are consumed there"""
    A, B = cls(kind), cls(kind, prefill=False)
    ka, va, dka, dva = batch(A, 3000, 19)
    kb, vb, dkb, dvb = batch(B, 3000, 23)
    kb[:500] = ka[:500]                                        # keys both tables hold
    with torch.cuda.stream(s1):
        bk, bv = late_inputs(s1, (kb, dkb), (vb, dvb))
        assert_busy(s1)
        assert B.g.insert(bk, bv) == B.o.insert(kb, vb)
    with torch.cuda.stream(s2):
        bk, bv = late_inputs(s2, (ka, dka), (va, dva))
        assert_busy(s2)
        assert A.g.insert(bk, bv) == A.o.insert(ka, va)
        sk, sv = consume_on(s2, *B.g.select_values(0, M32, device=True))
        hk, hv = B.g.to_vector()
        assert np.array_equal(u64(sk), hk) and np.array_equal(u32(sv), hv)
        exp, other = A.items(), B.items()
        n_new = A.g.merge(B.g, "plus")
    for kk, vv in other.items():
        exp[kk] = (exp[kk] + vv) & M32 if kk in exp else vv
    assert n_new == len(exp) - len(A.items())
    for a, b in zip(A.g.sorted_items(), A.sorted_arrays(exp)):
        assert np.array_equal(a, b)
    B.check()
    A.close(); B.close()


# ---- A. indexes -------------------------------------------------------------------------------------------------------------------
K_NARROW, K_WIDE = 21, 40


class Idx:
    """an index of either key width with the pairs of TEXT and the model of them"""

    def __init__(self, wide, **kw):
        self.wide = wide
        self.k = K_WIDE if wide else K_NARROW
        self.x = (WideKmerPositionIndex if wide else KmerPositionIndex)(self.k, True, **kw)
        self.Model = WideIndexModel if wide else IndexModel

    def pairs(self, text):
        pos = np_window_positions(text, self.k)
        km = np_kmers128(text, self.k, True) if self.wide else np_kmers(text, self.k, True)
        assert len(km) == len(pos)
        return np.ascontiguousarray(km), pos

    def decoy_pairs(self, n, seed):
        """n other valid k-mers with positions in range"""
        if self.wide:
            km = wide_rows(n, seed)
            km[:, 1] &= np.uint64((1 << (2 * self.k - 64)) - 1)
        else:
            km = W.distinct_u64(n, seed=seed) & np.uint64((1 << (2 * self.k)) - 1)
        return np.ascontiguousarray(km), np.random.default_rng(seed).integers(0, TEXT_N, n, dtype=np.uint64).astype(np.uint32)

    def check(self, km, pos):
        m = self.Model(km, pos)
        assert (self.x.size(), self.x.total()) == (m.size(), m.total())
        keys, offs, p = self.x.export()
        eo, ep = m.export_in_key_order(keys)
        assert np.array_equal(offs, eo) and np.array_equal(p, ep)
        return m

    def close(self):
        self.x.close()


WIDTHS = pytest.mark.parametrize("wide", [False, True], ids=["k21", "k40"])


@WIDTHS
def test_a_index_build_from_device_pairs(s, wide):
    I = Idx(wide)
    km, pos = I.pairs(TEXT)
    dk, dp = I.decoy_pairs(len(pos), 31)
    twin = Idx(wide)
    rehearse(s, lambda: twin.x.build(to_dev(dk), to_dev(dp)))
    twin.close()
    with torch.cuda.stream(s):
        bk, bp = late_inputs(s, (km, dk), (pos, dp))
        assert_busy(s)
        I.x.build(bk, bp)
    I.check(km, pos)
    I.close()


@WIDTHS
def test_a_index_build_sequences_from_device_text(s, wide):
    I = Idx(wide)
    twin = Idx(wide)
    rehearse(s, lambda: twin.x.build_sequences(to_dev(TEXT_DECOY)))
    twin.close()
    with torch.cuda.stream(s):
        bt = late_input(s, TEXT, TEXT_DECOY)
        assert_busy(s)
        n = I.x.build_sequences(bt)
    km, pos = I.pairs(TEXT)
    assert n == len(pos)
    I.check(km, pos)
    I.close()


def test_a_index_build_sequences_minimizers(s):
    I, twin = Idx(False, w=10), Idx(False, w=10)
    rehearse(s, lambda: twin.x.build_sequences(to_dev(TEXT_DECOY)))
    twin.close()
    with torch.cuda.stream(s):
        bt = late_input(s, TEXT, TEXT_DECOY)
        assert_busy(s)
        I.x.build_sequences(bt)
    I.check(*np_minimizers(TEXT, K_NARROW, 10, True, MURMUR, 42))
    I.close()


def test_a_index_build_sequences_syncmers(s):
    I, twin = Idx(True, s=25), Idx(True, s=25)
    rehearse(s, lambda: twin.x.build_sequences(to_dev(TEXT_DECOY)))
    twin.close()
    with torch.cuda.stream(s):
        bt = late_input(s, TEXT, TEXT_DECOY)
        assert_busy(s)
        I.x.build_sequences(bt)
    I.check(*np_syncmers(TEXT, K_WIDE, 25, True, MURMUR, 42, wide=True))
    I.close()


@WIDTHS
def test_a_index_append_and_erase(s, wide):
    I = Idx(wide)
    km, pos = I.pairs(TEXT)
    h = len(pos) // 2
    I.x.build(km[:h], pos[:h])
    dk, dp = I.decoy_pairs(len(pos) - h, 37)
    twin = Idx(wide)
    twin.x.build(km[:h], pos[:h])
    rehearse(s, lambda: (twin.x.append(to_dev(dk), to_dev(dp)), twin.x.erase(to_dev(np.ascontiguousarray(np.resize(km, (2 * len(km[::3]),) + km.shape[1:]))))))
    twin.close()
    with torch.cuda.stream(s):
        bk, bp = late_inputs(s, (km[h:], dk), (pos[h:], dp))
        assert_busy(s)
        I.x.append(bk, bp)
    I.check(km, pos)
    # erase: every third k-mer of the text and as many misses; the decoy erases other k-mers of the text
    e = np.ascontiguousarray(np.concatenate([km[::3], I.decoy_pairs(len(km[::3]), 41)[0]]))
    de = np.ascontiguousarray(np.resize(np.concatenate([km[1::3], km[2::3]]), e.shape))
    with torch.cuda.stream(s):
        be = late_input(s, e, de)
        assert_busy(s)
        nk, npos = I.x.erase(be)
    rows = km.reshape(len(km), -1)
    gone = {tuple(r) for r in e.reshape(len(e), -1).tolist()}
    keep = np.array([tuple(r) not in gone for r in rows.tolist()])
    m = I.check(km[keep], pos[keep])
    assert npos == len(pos) - int(keep.sum()) and nk == I.Model(km, pos).size() - m.size()
    I.close()


@WIDTHS
def test_a_index_count_and_find(s, wide):
    I = Idx(wide)
    km, pos = I.pairs(TEXT)
    I.x.build(km, pos)
    m = I.Model(km, pos)
    miss = I.decoy_pairs(1500, 43)[0]
    q = np.ascontiguousarray(np.concatenate([km[:1500], miss])[np.random.default_rng(5).permutation(3000)])
    dq = np.ascontiguousarray(np.concatenate([miss, km[4000:5500]]))
    rehearse(s, lambda: (I.x.count(to_dev(dq)), I.x.find(to_dev(dq))))
    with torch.cuda.stream(s):
        bq = late_input(s, q, dq)
        assert_busy(s)
        got = consume_on(s, I.x.count(bq))
        assert np.array_equal(u32(got), m.count(q))
    with torch.cuda.stream(s):
        bq = late_input(s, q, dq)
        assert_busy(s)
        offs, p = consume_on(s, *I.x.find(bq))
        eo, ep = m.find(q)
        assert np.array_equal(u64(offs), eo) and np.array_equal(u32(p), ep)
    I.close()


# ---- A. free functions ------------------------------------------------------------------------------------------------------------
def test_a_hash_batch(s):
    k, dk = W.distinct_u64(20_000, seed=51), W.distinct_u64(20_000, seed=52)
    rehearse(s, lambda: kh.hash_batch(to_dev(dk), "murmur3avx64", 43))
    with torch.cuda.stream(s):
        b = late_input(s, k, dk)
        assert_busy(s)
        got = consume_on(s, kh.hash_batch(b, "murmur3avx64", 43))
    assert np.array_equal(u64(got), O.hash_batch(O.HASH_MURMUR3_X86, 43, k))


def test_a_hash_batch_wide(s):
    k, dk = wide_rows(20_000, 53), wide_rows(20_000, 54)
    rehearse(s, lambda: KW.hash_batch_wide(to_dev(dk), "murmur3avx64", 43))
    with torch.cuda.stream(s):
        b = late_input(s, k, dk)
        assert_busy(s)
        got = consume_on(s, KW.hash_batch_wide(b, "murmur3avx64", 43))
    assert np.array_equal(u64(got), O.hash16_batch(O.HASH_MURMUR3_X86, 43, k))


@pytest.mark.parametrize("form", ["sequence", "sequence_pos", "fastq", "fastq_pos", "k128"])
def test_a_kmer_front_ends(s, form):
    fastq = form.startswith("fastq")
    text, decoy = (FASTQ, FASTQ_DECOY) if fastq else (TEXT, TEXT_DECOY)
    rehearse(s, lambda: KW.kmers128_from_sequence(to_dev(decoy), K_WIDE, True) if form == "k128" else
             KM.kmers_from_sequence(to_dev(decoy), K_NARROW, True, _fastq=fastq, with_positions=form.endswith("_pos")))
    with torch.cuda.stream(s):
        b = late_input(s, text, decoy)
        assert_busy(s)
        if form == "k128":
            got = [consume_on(s, KW.kmers128_from_sequence(b, K_WIDE, True))]
            exp = [np_kmers128(text, K_WIDE, True)]
        elif form.endswith("_pos"):
            got = consume_on(s, *(KM.kmers_from_fastq if fastq else KM.kmers_from_sequence)(b, K_NARROW, True, with_positions=True))
            exp = (np_kmers_fastq_pos if fastq else np_kmers_pos)(text, K_NARROW, True)
        else:
            got = [consume_on(s, (KM.kmers_from_fastq if fastq else KM.kmers_from_sequence)(b, K_NARROW, True))]
            exp = [(np_kmers_fastq if fastq else np_kmers)(text, K_NARROW, True)]
    assert np.array_equal(u64(got[0]), exp[0])
    if len(exp) == 2:
        assert np.array_equal(u32(got[1]), exp[1])


@pytest.mark.parametrize("form", ["minimizers", "syncmers", "syncmers128"])
def test_a_samplers(s, form):
    rehearse(s, lambda: {"minimizers": lambda t: KM.minimizers_from_sequence(t, 15, 10, True, "murmur", 42),
                         "syncmers": lambda t: KM.syncmers_from_sequence(t, 15, 11, True, "murmur", 42),
                         "syncmers128": lambda t: KW.syncmers128_from_sequence(t, K_WIDE, 25, True, "murmur", 42)}[form](to_dev(TEXT_DECOY)))
    with torch.cuda.stream(s):
        b = late_input(s, TEXT, TEXT_DECOY)
        assert_busy(s)
        if form == "minimizers":
            km, pos = consume_on(s, *KM.minimizers_from_sequence(b, 15, 10, True, "murmur", 42))
            ek, ep = np_minimizers(TEXT, 15, 10, True, MURMUR, 42)
        elif form == "syncmers":
            km, pos = consume_on(s, *KM.syncmers_from_sequence(b, 15, 11, True, "murmur", 42))
            ek, ep = np_syncmers(TEXT, 15, 11, True, MURMUR, 42)
        else:
            km, pos = consume_on(s, *KW.syncmers128_from_sequence(b, K_WIDE, 25, True, "murmur", 42))
            ek, ep = np_syncmers(TEXT, K_WIDE, 25, True, MURMUR, 42, wide=True)
    assert len(ek) and np.array_equal(u64(km), ek) and np.array_equal(u32(pos), ep)


@pytest.mark.parametrize("wide", [False, True], ids=["k15", "k40"])
def test_a_is_syncmer(s, wide):
    k, sm = (K_WIDE, 25) if wide else (15, 11)
    km = (np_kmers128 if wide else np_kmers)(TEXT, k, True)
    q, dq = np.ascontiguousarray(km[:2000]), np.ascontiguousarray(km[3000:5000])
    rehearse(s, lambda: (KW.is_syncmer128 if wide else KM.is_syncmer)(to_dev(dq), k, sm, True, "murmur", 42))
    with torch.cuda.stream(s):
        b = late_input(s, q, dq)
        assert_busy(s)
        got = consume_on(s, (KW.is_syncmer128 if wide else KM.is_syncmer)(b, k, sm, True, "murmur", 42))
    exp = np_is_syncmer(q, k, sm, True, MURMUR, 42)
    assert exp.any() and not exp.all() and np.array_equal(got, exp)


@pytest.mark.parametrize("wide", [False, True], ids=["u64", "wide"])
def test_a_shard_permute(s, wide):
    """the stable partition by destination rank that kmerhash_amd.dist sends its batches through"""
    from kmerhash_amd.dist import DIST_SEED, GpuBackend, WideGpuBackend
    n, p = 20_001, 4
    k, dk = (wide_rows(n, 61), wide_rows(n, 62)) if wide else (W.distinct_u64(n, seed=61), W.distinct_u64(n, seed=62))
    v = np.arange(n, dtype=np.uint32)
    be = (WideGpuBackend if wide else GpuBackend)(0)
    rehearse(s, lambda: be.shard(to_dev(dk), to_dev(v), p))
    with torch.cuda.stream(s):
        bk, bv = late_inputs(s, (k, dk), (v, v[::-1].copy()))
        assert_busy(s)
        ok, ov, counts = be.shard(bk, bv, p)
        ok, ov = consume_on(s, ok, ov)
    h = O.hash16_batch(O.HASH_MURMUR3_X86, DIST_SEED, k) if wide else O.hash_batch(O.HASH_MURMUR3_X86, DIST_SEED, k)
    r = (h % np.uint64(p)).astype(np.int64)
    order = np.argsort(r, kind="stable")
    assert counts == np.bincount(r, minlength=p).tolist()
    assert np.array_equal(u64(ok).reshape(k.shape), k[order]) and np.array_equal(u32(ov), v[order])
    be.table.close()


# ---- HyperLogLog ------------------------------------------------------------------------------------------------------------------
HLL_N = 20_000
PRECISIONS = pytest.mark.parametrize("precision", [12, 14], ids=["p12-lds", "p14-global"])      # registers in LDS / in global memory
HID = O.HASH_MURMUR3_X86


def hll_keys(seed):
    return W.distinct_u64(HLL_N, seed=seed)


def oracle_regs(precision, *hash_batches):
    o = O.OracleHLL(precision, 0, HID, 43)
    for hv in hash_batches:
        o.update_via_hashval(np.ascontiguousarray(hv))
    r = o.registers().copy()
    o.close()
    return r


def text_hashes(text, k, fastq=False):
    return O.hash_batch(HID, 43, (np_kmers_fastq if fastq else np_kmers)(text, k, True))


@PRECISIONS
@pytest.mark.parametrize("op", ["update", "update_via_hashval", "update_wide", "update_from_sequence", "update_from_fastq"])
def test_a_hll_updates(s, precision, op):
    h = hyperloglog64(precision, 0, "murmur3avx64", 43)
    with torch.cuda.stream(s):
        if op == "update_wide":
            k, dk = wide_rows(HLL_N, 71), wide_rows(HLL_N, 72)
            hv = O.hash16_batch(HID, 43, k)
        elif op.startswith("update_from"):
            fastq = op.endswith("fastq")
            k, dk = (FASTQ, FASTQ_DECOY) if fastq else (TEXT, TEXT_DECOY)
            hv = text_hashes(k, K_NARROW, fastq)
        else:
            k, dk = hll_keys(71), hll_keys(72)
            hv = O.hash_batch(HID, 43, k) if op == "update" else k
        twin = hyperloglog64(precision, 0, "murmur3avx64", 43)
        rehearse(s, lambda: (getattr(twin, op)(to_dev(dk), K_NARROW, True) if op.startswith("update_from") else getattr(twin, op)(to_dev(dk)),
                             twin.registers()))
        twin.close()
        b = late_input(s, k, dk)
        assert_busy(s)
        if op.startswith("update_from"):
            assert getattr(h, op)(b, K_NARROW, True) == len(hv)
        else:
            getattr(h, op)(b)
        got = h.registers()
    assert np.array_equal(got, oracle_regs(precision, hv))
    h.close()


def switch(h, stream, how):
    """the next call on `h` is made under `stream`: "python" leaves it to the host layer (which adopts torch's current stream only for
    calls with a device argument), "capi" switches the handle itself with kh_hll_set_stream"""
    if how == "capi":
        assert h._L.kh_hll_set_stream(h._h, C.c_void_p(stream.cuda_stream)) == 0


SWITCH = pytest.mark.parametrize("how", ["python", "capi"])


@PRECISIONS
@SWITCH
@pytest.mark.parametrize("then", ["registers", "clear", "update"])
def test_b_hll_stream_switch_after_a_device_update(s1, s2, precision, how, then):
    h = hyperloglog64(precision, 0, "murmur3avx64", 43)
    k, k2 = hll_keys(73), hll_keys(75)
    with torch.cuda.stream(s1):
        b = late_input(s1, k, hll_keys(74), beside=(s2,))
        assert_busy(s1)
        h.update(b)
    with torch.cuda.stream(s2):
        assert_busy(s1)
        switch(h, s2, how)
        if then == "registers":
            got, exp = h.registers(), oracle_regs(precision, O.hash_batch(HID, 43, k))
        elif then == "clear":
            h.clear()
            got, exp = h.registers(), np.zeros(1 << precision, dtype=np.uint8)
            s1.synchronize()                                   # a clear that overtook the update would be undone by it now
            assert np.array_equal(h.registers(), exp)
        else:
            h.update(to_dev(k2))
            got, exp = h.registers(), oracle_regs(precision, O.hash_batch(HID, 43, k), O.hash_batch(HID, 43, k2))
    assert np.array_equal(got, exp)
    h.close()


@PRECISIONS
@SWITCH
def test_b_hll_estimate_after_a_text_pass_on_another_stream(s1, s2, precision, how):
    h = hyperloglog64(precision, 0, "murmur3avx64", 43)
    o = O.OracleHLL(precision, 0, HID, 43)
    o.update_via_hashval(text_hashes(TEXT, K_NARROW))
    with torch.cuda.stream(s1):
        b = late_input(s1, TEXT, TEXT_DECOY, beside=(s2,))
        assert_busy(s1)
        # (the host layer asks for the window count, which waits; the C call with n_kmers == NULL does not)
        assert h._L.kh_hll_set_stream(h._h, C.c_void_p(s1.cuda_stream)) == 0
        assert h._L.kh_hll_update_from_sequence(h._h, b.data_ptr(), b.numel(), K_NARROW, 1, 1, None) == 0
    with torch.cuda.stream(s2):
        assert_busy(s1)
        switch(h, s2, how)
        assert h.estimate() == o.estimate()
    h.close(); o.close()


@PRECISIONS
def test_c_hll_merge_reads_the_other_estimator_after_its_pending_update(s1, s2, precision):
    a, b = hyperloglog64(precision, 0, "murmur3avx64", 43), hyperloglog64(precision, 0, "murmur3avx64", 43)
    ka, kb = hll_keys(76), hll_keys(77)
    a.update(ka)
    with torch.cuda.stream(s1):
        buf = late_input(s1, kb, hll_keys(78), beside=(s2,))
        assert_busy(s1)
        b.update(buf)
    with torch.cuda.stream(s2):
        assert_busy(s1)
        a.merge(b)
        got = a.registers()
    assert np.array_equal(got, oracle_regs(precision, O.hash_batch(HID, 43, ka), O.hash_batch(HID, 43, kb)))
    assert np.array_equal(b.registers(), oracle_regs(precision, O.hash_batch(HID, 43, kb)))
    a.close(); b.close()


# ---- B. one table / index, two streams --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,kind", TABLES, ids=[t[0] for t in TABLES])
def test_b_table_insert_on_one_stream_queries_on_another(s1, s2, name, cls, kind):
    T = cls(kind)
    k, v, dk, dv = batch(T, 3000, 81)
    with torch.cuda.stream(s1):
        bk, bv = late_inputs(s1, (k, dk), (v, dv))
        assert_busy(s1)
        assert T.g.insert(bk, bv) == T.o.insert(k, v)
    q = np.ascontiguousarray(np.concatenate([k[:500], dk[:500], T.base[:500]]))
    with torch.cuda.stream(s2):
        bq = late_input(s2, q, q[::-1].copy())
        assert_busy(s2)
        got = consume_on(s2, T.g.count(bq))
        assert np.array_equal(got, T.o.count(q))
        fk, fv = consume_on(s2, *T.g.find(to_dev(q)))
        ek, ev = T.o.find_compact(q) if cls is Narrow else T.o.find(q)
        assert np.array_equal(u64(fk).reshape(ek.shape), ek) and np.array_equal(u32(fv), ev)
    T.check()
    T.close()


@pytest.mark.parametrize("name,cls,kind", TABLES, ids=[t[0] for t in TABLES])
def test_b_table_pending_count_then_erase_on_another_stream(s1, s2, name, cls, kind):
    """count with device queries leaves its kernel pending on s1; an erase of the same keys issued at once under s2 must not overtake
    it, and to_vector() with no stream context sees the erase"""
    T = cls(kind)
    q, dq = queries(T, 3000, 83)
    rehearse(s1, lambda: T.g.count(to_dev(dq)))
    exp_count = T.o.count(q)          # (the models are slow: nothing but the two calls stands between the two busy checks)
    eq = to_dev(q)
    with torch.cuda.stream(s1):
        bq = late_input(s1, q, dq, beside=(s2,))
        assert_busy(s1)
        pending = T.g.count(bq)
    with torch.cuda.stream(s2):
        assert_busy(s1)
        n_erased = T.g.erase(eq)
    assert n_erased == T.o.erase(q)
    assert np.array_equal(consume_on(s1, pending), exp_count) and exp_count.any()
    gk, gv = T.g.to_vector()
    ek, ev = T.o.sorted_items()
    o = np.lexsort((gk[:, 0], gk[:, 1])) if T.wide else np.argsort(gk, kind="stable")
    assert np.array_equal(gk[o], ek) and np.array_equal(gv[o], ev)
    T.close()


@pytest.mark.parametrize("name,cls,kind", TABLES, ids=[t[0] for t in TABLES])
def test_b_streamed_insert_fed_on_one_stream_ended_on_another(s1, s2, name, cls, kind):
    T = cls(kind, prefill=False)
    k, v, dk, dv = batch(T, 20_000, 85)
    with torch.cuda.stream(s1):
        T.g.insert_begin(20_000)
        bk, bv = late_inputs(s1, (k[:12_000], dk[:12_000]), (v[:12_000], dv[:12_000]))
        assert_busy(s1)
        T.g.insert_feed(bk, bv)
    with torch.cuda.stream(s2):
        assert_busy(s1)
        T.g.insert_feed(to_dev(k[12_000:]), to_dev(v[12_000:]))
        assert T.g.insert_end() == T.o.insert(k, v)
    T.check()
    T.close()


@WIDTHS
def test_b_index_build_on_one_stream_queries_and_erase_on_others(s1, s2, wide):
    I = Idx(wide)
    km, pos = I.pairs(TEXT)
    dk, dp = I.decoy_pairs(len(pos), 87)
    with torch.cuda.stream(s1):
        bk, bp = late_inputs(s1, (km, dk), (pos, dp))
        assert_busy(s1)
        I.x.build(bk, bp)
    m = I.Model(km, pos)
    q = np.ascontiguousarray(np.concatenate([km[:1000], dk[:1000]]))
    with torch.cuda.stream(s2):
        bq = late_input(s2, q, q[::-1].copy())
        assert_busy(s2)
        assert np.array_equal(u32(consume_on(s2, I.x.count(bq))), m.count(q))
        offs, p = consume_on(s2, *I.x.find(to_dev(q)))
        eo, ep = m.find(q)
        assert np.array_equal(u64(offs), eo) and np.array_equal(u32(p), ep)
    e = np.ascontiguousarray(km[::2])
    with torch.cuda.stream(s1):
        be = late_input(s1, e, np.ascontiguousarray(np.resize(km[1::2], e.shape)))
        assert_busy(s1)
        I.x.erase(be)
    gone = {tuple(r) for r in e.reshape(len(e), -1).tolist()}
    keep = np.array([tuple(r) not in gone for r in km.reshape(len(km), -1).tolist()])
    I.check(km[keep], pos[keep])          # export() with no stream context
    I.close()


# ---- C. two tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,kind", TABLES, ids=[t[0] for t in TABLES])
def test_c_table_merge_source_filled_on_another_stream(s1, s2, name, cls, kind):
    """src is filled under s1 and still has a count pending there when dst.merge(src) is called under s2"""
    dst, src = cls(kind), cls(kind, prefill=False)
    k, v, dk, dv = batch(src, 5000, 91)
    with torch.cuda.stream(s1):
        bk, bv = late_inputs(s1, (k, dk), (v, dv))
        assert_busy(s1)
        assert src.g.insert(bk, bv) == src.o.insert(k, v)
        pending = src.g.count(late_input(s1, k, dk))          # leaves work of src pending on s1
    with torch.cuda.stream(s2):
        assert_busy(s1)
        exp, before = dst.items(), len(dst.items())
        n_new = dst.g.merge(src.g, "max")
    for kk, vv in src.items().items():
        exp[kk] = max(exp[kk], vv) if kk in exp else vv
    assert n_new == len(exp) - before
    for a, b in zip(dst.g.sorted_items(), dst.sorted_arrays(exp)):
        assert np.array_equal(a, b)
    assert consume_on(s1, pending).all()
    src.check()
    dst.close(); src.close()


# ---- D. the sharded table's pipeline under a caller's side stream ----------------------------------------------------------------
def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _d_worker(port, q):
    """one rank over RCCL with forced collectives (as tests/test_gpu_dist_nccl.py): ShardedTable takes the multi-rank route -- shard
    plan, per-piece permutation on the caller's stream, exchanges on the comm side stream, streamed insert, pipelined queries"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        from kmerhash_amd import dist as khd
        assert khd.FORCE_COLLECTIVES
        keys, vals = W.w1_benchmark_hashtables(50_000, seed=12)
        dkeys, dvals = W.distinct_u64(50_000, seed=95), vals[::-1].copy()
        s = side_stream()
        warm = khd.ShardedTable(khd.GpuBackend(0))          # the first collectives set the communicator up: not inside a delay
        with torch.cuda.stream(s):
            warm.insert(to_dev(dkeys), to_dev(dvals), chunks=4)
            warm.find(to_dev(dkeys[:4000]))
            warm.synchronize()
        warm.local.close()
        st = khd.ShardedTable(khd.GpuBackend(0))
        assert not st._single()
        o = O.OracleTable(0, 128, 0.35, 0.8)
        with torch.cuda.stream(s):
            bk, bv = late_inputs(s, (keys, dkeys), (vals, dvals))
            assert_busy(s)
            assert st.insert(bk, bv, chunks=4) == o.insert(keys, vals)
        assert st.collectives == {"counts": 1, "payload": 4, "votes": 3}, st.collectives
        for a, b in zip(st.local.sorted_items(), o.sorted_items()):
            assert np.array_equal(a, b)
        q1 = np.ascontiguousarray(np.concatenate([keys[:10_000], dkeys[:10_000]])[W.shuffle_perm(20_000, 3)])
        st.query_pieces = 3
        for op in ("find", "count"):
            c0 = dict(st.collectives)
            with torch.cuda.stream(s):
                bq = late_input(s, q1, q1[::-1].copy())
                assert_busy(s)
                res = consume_on(s, *getattr(st, op)(bq))          # no host wait between the call and the consumer on s
            st.synchronize()
            pieces = 6          # per piece one key exchange and one result exchange
            assert st.collectives == {"counts": c0["counts"] + 1, "payload": c0["payload"] + pieces, "votes": c0["votes"] + 1}, (op, st.collectives)
            assert np.array_equal(u64(res[0]), q1)                 # the permuted order of ONE rank is the input order
            if op == "find":
                ev, ef = o.find(q1)
                assert np.array_equal(res[2], ef) and np.array_equal(u32(res[1])[ef == 1], ev[ef == 1]) and ef.any() and not ef.all()
            else:
                assert np.array_equal(res[1], o.count(q1))
        sc = khd.ShardedTable(khd.GpuBackend(0))
        uk, cnt = np.unique(keys, return_counts=True)
        with torch.cuda.stream(s):
            bk = late_input(s, keys, dkeys)
            assert_busy(s)
            assert sc.insert_counts(bk, chunks=4) == len(uk)
        assert sc.collectives == {"counts": 1, "payload": 4, "votes": 3}, sc.collectives
        sk, sv = sc.local.sorted_items()
        assert np.array_equal(sk, uk) and np.array_equal(sv, cnt.astype(np.uint32))
        q.put("ok")
    except Exception:  # pragma: no cover
        import traceback
        q.put("FAIL: " + traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_d_sharded_table_pipeline_on_a_side_stream(monkeypatch):
    """insert(chunks=4), insert_counts(chunks=4) and the pipelined find / count (3 pieces) of a ShardedTable that runs its exchanges on
    its own comm stream, called under a caller's side stream with late inputs, results consumed on that stream; the collective counts
    pin the route.  A child process: the process group and the forced collectives are its own."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("KH_DIST_FORCE_COLLECTIVES", "1")          # read by kmerhash_amd.dist when the child imports it
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_d_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=300)
    p.join(60)
    assert res == "ok", res
