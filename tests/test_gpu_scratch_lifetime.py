"""GPU: a temporary block of the process-wide device pool goes back only after the queued work that uses it has run.

pool_free puts a block on the free list at once and pool_alloc, on any stream, takes the first block that fits: a block handed back while
a queued kernel still reads it is overwritten by the next call.  On the null stream, where the model comparisons run, that cannot show.
Every case here follows one recipe (helpers: tests/stream_checks.py):

    1. wait for the device and empty the pool (kh_release_cached_memory): a premature free can then only hand out the block under test
    2. hold stream A with a delay and issue call A on it -- a call that only queues its work, so it returns while the delay runs
    3. on a stream B that runs beside A, issue call B: the same entry point and shapes (the same scratch size) over other well-formed
       data, and wait for B alone
    4. assert_busy(A): A was still pending while B ran to completion
    5. read A's results in the order of stream A and compare A's AND B's outputs, bit for bit, with values that do not come from the library

If B's scratch replaced A's, A computes a wrong answer from valid numbers.  Every output has a guard (GUARD bytes) that must stay untouched.

A call that fills its scratch on its own stream before it reads it comes out right even from a shared block, and so does B.  The cases
of such calls therefore add a WITNESS: a shard plan made on stream B right after A was issued.  Its scanned offsets live in its block
until it is destroyed; it takes A's block if A gave it back too early, A then runs over it, and the witness is permuted and checked
only after A has drained.

The release path each case guards:
    shard plan, permute / permute_global, with and without values: kh_shard_plan_destroy -- the host function queued behind the scatters
    shard plan, the two pieces on two held streams: kh_shard_plan_destroy -- one host function per stream, the last to run frees
    shard plan destroyed on a capturing stream: kh_shard_plan_destroy -- no host node, the block is freed once and not at every replay
    chain_edits: Scratch::finish_queued -- the block of the worklist must not reach the witness before k_edits_classify / k_edits_wfa ran
    select_chains: Scratch::finish_queued -- the block of k_select_block's sort arrays (a group of more than 2048 chains), likewise
    pair_chains: Scratch::finish_queued with device inputs -- the call takes no pooled block; pinned: it returns at once and is right
    pack_rows: Scratch::finish_queued with device inputs -- the call takes no pooled block; pinned: it returns at once and is right
All four also pin "returns without a wait": assert_busy fails if finish_queued falls back to finish().
The shared tail of the count-scan-emit calls (emit_total) waits for its stream before it queues the emit kernels: it cannot return
while a delay runs, so the recipe does not reach it."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402
from kmerhash_amd._call import TORCH_DTYPE  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
import edits_model as EM  # noqa: E402
import fastq_cases as FC  # noqa: E402
import fastq_model as FM  # noqa: E402
import select_cases as SC  # noqa: E402
from edits_cases import Batch, bases, sub  # noqa: E402
from pair_cases import random_table  # noqa: E402
from pair_model import pair_model  # noqa: E402
from select_model import select_model  # noqa: E402
from stream_checks import assert_busy, consume_on, delay, side_stream, to_dev  # noqa: E402

GUARD = 0x5A
DIST_SEED = 9876543
TILE = 4096                       # pairs per tile of the shard kernels (8-byte keys)
N = 2 * TILE + 777                # three tiles, the last one ragged
P, PIECES = 3, 2


def empty_pool():
    torch.cuda.synchronize()
    assert K.lib().kh_release_cached_memory(0) == K.KH_OK


@pytest.fixture(scope="module")
def streams():
    a = side_stream()
    return a, side_stream(a)


@pytest.fixture(scope="module")
def third_stream(streams):
    return side_stream(*streams)


# ---- a. the shard plan through the C API --------------------------------------------------------------------------------------------
def plan_keys(seed):
    keys = W.splitmix64(np.arange(N, dtype=np.uint64) + np.uint64(seed * 1_000_003))
    keys[::7] = keys[0]                                   # duplicates
    return keys, (np.arange(N, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)).astype(np.uint32)


def grouped(keys, vals, lo, hi):
    """the stable grouping by rank of the pairs [lo, hi): the definition of the permutation, from the CPU oracle's hash"""
    rank = (O.hash_batch(O.HASH_MURMUR3_X86, DIST_SEED, keys[lo:hi]) % np.uint64(P)).astype(np.int64)
    order = np.argsort(rank, kind="stable")
    return keys[lo:hi][order], vals[lo:hi][order]


def plan_expected(keys, vals, bounds, glob):
    if glob:
        return grouped(keys, vals, 0, N)
    parts = [grouped(keys, vals, bounds[i], bounds[i + 1]) for i in range(PIECES)]      # piece i goes to out + bounds[i]
    return np.concatenate([k for k, _ in parts]), np.concatenate([v for _, v in parts])


class PlanOut:
    """key and value outputs of one plan inside guards.  A scatter driven by the offsets of ANOTHER plan of the same n lands within
    [-n, 3n + TILE) of the output's start (a rank offset is at most n off, the adjustment of a piece at most n, the piece's place n),
    so with HEAD = 2n and TAIL = 4n entries even that stays inside the buffer."""
    HEAD, TAIL = 2 * N, 4 * N

    def __init__(self, with_vals):
        self.k = torch.full((self.HEAD + N + self.TAIL,), GUARD, dtype=torch.int64, device="cuda")
        self.v = torch.full((self.HEAD + N + self.TAIL,), GUARD, dtype=torch.int32, device="cuda") if with_vals else None

    def ptrs(self, at):
        return self.k[self.HEAD + at:].data_ptr(), (self.v[self.HEAD + at:].data_ptr() if self.v is not None else None)

    def check(self, k, v, exp, who):
        h, e = self.HEAD, self.HEAD + N
        assert (k[:h] == GUARD).all() and (k[e:] == GUARD).all(), "%s: keys written outside the output" % who
        assert np.array_equal(k[h:e].view(np.uint64), exp[0]), "%s: wrong key permutation (guards intact)" % who
        if v is not None:
            assert (v[:h] == GUARD).all() and (v[e:] == GUARD).all(), "%s: values written outside the output" % who
            assert np.array_equal(v[h:e].view(np.uint32), exp[1]), "%s: wrong value permutation (guards intact)" % who


def plan_create(dk, stream):
    L = K.lib()
    plan = C.c_void_p()
    counts, bounds = (C.c_uint64 * (P * PIECES))(), (C.c_uint64 * (PIECES + 1))()
    assert L.kh_shard_plan_create(C.byref(plan), 1, DIST_SEED, 0, 0, P, dk.data_ptr(), N, PIECES, counts, bounds, 0, stream.cuda_stream) == K.KH_OK
    bounds = [int(b) for b in bounds]
    assert bounds == [0, TILE, N]
    return plan, bounds


def plan_permute(plan, bounds, dk, dv, out, stream, glob):
    L = K.lib()
    fn = L.kh_shard_plan_permute_global if glob else L.kh_shard_plan_permute
    for i in range(PIECES):
        ok, ov = out.ptrs(0 if glob else bounds[i])
        assert fn(plan, i, dk.data_ptr(), dv.data_ptr() if dv is not None else None, ok, ov, stream.cuda_stream) == K.KH_OK


@pytest.mark.parametrize("with_vals", [True, False], ids=["values", "keys_only"])
@pytest.mark.parametrize("glob", [False, True], ids=["permute", "permute_global"])
def test_shard_plan_block_outlives_its_queued_permutes(streams, glob, with_vals):
    sa, sb = streams
    L = K.lib()
    (ka, va), (kb, vb) = plan_keys(1), plan_keys(2)
    dka, dkb = to_dev(ka), to_dev(kb)
    dva, dvb = (to_dev(va), to_dev(vb)) if with_vals else (None, None)
    oa, ob = PlanOut(with_vals), PlanOut(with_vals)
    try:
        empty_pool()
        plan_a, bounds = plan_create(dka, sa)                    # (create waits for its stream: before the delay)
        delay(sa)
        plan_permute(plan_a, bounds, dka, dva, oa, sa, glob)
        L.kh_shard_plan_destroy(plan_a)                          # the permutes have returned; they are still queued
        plan_b, bounds_b = plan_create(dkb, sb)
        plan_permute(plan_b, bounds_b, dkb, dvb, ob, sb, glob)
        sb.synchronize()
        assert_busy(sa)                                          # A was pending while B was planned, permuted and completed
        L.kh_shard_plan_destroy(plan_b)
        got_a = consume_on(sa, oa.k, oa.v)
        got_b = [ob.k.cpu().numpy(), ob.v.cpu().numpy() if with_vals else None]
        oa.check(*got_a, plan_expected(ka, va, bounds, glob), "plan A (destroyed with its permutes queued)")
        ob.check(*got_b, plan_expected(kb, vb, bounds, glob), "plan B")
    finally:
        torch.cuda.synchronize()


def test_shard_plan_block_outlives_permutes_on_two_streams(streams, third_stream):
    """piece 0 is queued on stream A and piece 1 on a third stream, each behind its own delay; the plan is destroyed at once.  Either
    stream alone must keep the block: B is planned and permuted while both are held."""
    sa, sb = streams
    sc = third_stream
    L = K.lib()
    (ka, va), (kb, vb) = plan_keys(7), plan_keys(8)
    dka, dva, dkb, dvb = (to_dev(x) for x in (ka, va, kb, vb))
    oa, ob = PlanOut(True), PlanOut(True)
    try:
        empty_pool()
        plan_a, bounds = plan_create(dka, sa)
        delay(sa)
        delay(sc)
        for i, st in enumerate((sa, sc)):
            ok, ov = oa.ptrs(0)
            assert L.kh_shard_plan_permute_global(plan_a, i, dka.data_ptr(), dva.data_ptr(), ok, ov, st.cuda_stream) == K.KH_OK
        L.kh_shard_plan_destroy(plan_a)
        plan_b, bounds_b = plan_create(dkb, sb)
        plan_permute(plan_b, bounds_b, dkb, dvb, ob, sb, True)
        sb.synchronize()
        assert_busy(sa)
        assert_busy(sc)                                          # both pieces of A were pending while B completed
        L.kh_shard_plan_destroy(plan_b)
        sc.synchronize()
        got_a = consume_on(sa, oa.k, oa.v)
        oa.check(*got_a, plan_expected(ka, va, bounds, True), "plan A (pieces on two streams)")
        ob.check(ob.k.cpu().numpy(), ob.v.cpu().numpy(), plan_expected(kb, vb, bounds, True), "plan B")
    finally:
        torch.cuda.synchronize()


def test_shard_plan_never_permuted_or_empty_frees_at_once(streams):
    """a plan that queued nothing has nothing to wait for: destroyed under a running delay, its block is the next plan's at once (the
    pool was empty, so the second create would otherwise have to ask the driver: not observable; what is: both calls return while the
    delay runs and the second plan is right)"""
    sa, sb = streams
    L = K.lib()
    ka, va = plan_keys(3)
    dka, dva = to_dev(ka), to_dev(va)
    out = PlanOut(True)
    try:
        empty_pool()
        idle, _ = plan_create(dka, sa)
        none = C.c_void_p()
        counts, bounds = (C.c_uint64 * (P * PIECES))(), (C.c_uint64 * (PIECES + 1))()
        assert L.kh_shard_plan_create(C.byref(none), 1, DIST_SEED, 0, 0, P, None, 0, PIECES, counts, bounds, 0, sa.cuda_stream) == K.KH_OK
        assert L.kh_shard_plan_permute(none, 0, None, None, None, None, sa.cuda_stream) == K.KH_OK
        delay(sa)
        L.kh_shard_plan_destroy(idle)
        L.kh_shard_plan_destroy(none)
        L.kh_shard_plan_destroy(None)
        assert_busy(sa)
        plan, b = plan_create(dka, sb)
        plan_permute(plan, b, dka, dva, out, sb, True)
        L.kh_shard_plan_destroy(plan)
        sb.synchronize()
        assert_busy(sa)
        out.check(out.k.cpu().numpy(), out.v.cpu().numpy(), plan_expected(ka, va, b, True), "plan after an idle one")
    finally:
        torch.cuda.synchronize()


# ---- e. destroy on a capturing stream -------------------------------------------------------------------------------------------------
def test_shard_plan_destroyed_during_capture_is_freed_once(streams):
    """the permutes of a plan are captured into a graph (one stream: no parallel branches) and the plan is destroyed inside the capture:
    nothing is queued for the block -- a host node would hand it back at every replay, and two later plans would then share it.  After
    two replays two plans that live at the same time both permute correctly."""
    sa, _ = streams
    L = K.lib()
    (ka, va), (kb, vb), (kc, vc) = plan_keys(4), plan_keys(5), plan_keys(6)
    dka, dva, dkb, dvb, dkc, dvc = (to_dev(x) for x in (ka, va, kb, vb, kc, vc))
    oa, ob, oc = PlanOut(True), PlanOut(True), PlanOut(True)
    try:
        empty_pool()
        plan_a, bounds = plan_create(dka, sa)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=sa):
            plan_permute(plan_a, bounds, dka, dva, oa, sa, True)
            L.kh_shard_plan_destroy(plan_a)
        # The replays below read a block that already sits in the pool's free list.  That is right here only because nothing takes a
        # block in between; it is not how the call is meant to be used (the header: destroy such a plan after the last replay).  The
        # test destroys inside the capture because that is the one place where a host node could be recorded by mistake.
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        oa.check(oa.k.cpu().numpy(), oa.v.cpu().numpy(), plan_expected(ka, va, bounds, True), "the replayed plan")
        plan_b, bb = plan_create(dkb, sa)
        plan_c, bc = plan_create(dkc, sa)                        # both alive: a block that sat in the pool twice would be shared
        plan_permute(plan_b, bb, dkb, dvb, ob, sa, True)
        plan_permute(plan_c, bc, dkc, dvc, oc, sa, True)
        L.kh_shard_plan_destroy(plan_b)
        L.kh_shard_plan_destroy(plan_c)
        got = consume_on(sa, ob.k, ob.v, oc.k, oc.v)
        ob.check(got[0], got[1], plan_expected(kb, vb, bb, True), "first plan after the replays")
        oc.check(got[2], got[3], plan_expected(kc, vc, bc, True), "second plan after the replays")
    finally:
        torch.cuda.synchronize()


# ---- d. the finish_queued callers with device inputs ------------------------------------------------------------------------------------
class Guarded:
    """stands in for the output allocation of the Python calls: every output gets a tail of TAIL guard bytes"""
    TAIL = 4096

    def __init__(self):
        self.bufs = []

    def alloc(self, like, shape, np_dtype, zero=False, empty=False):
        assert like.where == K.KH_MEM_DEVICE
        used = int(shape) * np.dtype(np_dtype).itemsize
        raw = torch.full((used + self.TAIL,), GUARD, dtype=torch.uint8, device=like.device)
        if zero:
            raw[:used].zero_()
        t = raw[:used].view(TORCH_DTYPE[np_dtype])
        self.bufs.append((raw, used))
        return t, (None if empty and used == 0 else t.data_ptr())

    def check(self):
        assert self.bufs
        for raw, used in self.bufs:
            assert (raw[used:] == GUARD).all(), "a call wrote behind its output"


@pytest.fixture
def guarded(monkeypatch):
    g = Guarded()
    monkeypatch.setattr("kmerhash_amd.mapper.alloc", g.alloc)
    monkeypatch.setattr("kmerhash_amd.fastq.alloc", g.alloc)
    return g


def queued_pair(streams, guarded, call, args_a, args_b, exp_a, exp_b):
    """the recipe for a Python call: call(*device arguments) -> tuple of device results; exp_*: the models' arrays in the same order.
    Between A and B the witness plan is made on stream B (the module's docstring); it is permuted after A has drained."""
    sa, sb = streams
    L = K.lib()
    kw, vw = plan_keys(9)
    dkw, dvw = to_dev(kw), to_dev(vw)
    ow = PlanOut(True)
    da, db = [to_dev(x) if isinstance(x, np.ndarray) else x for x in args_a], [to_dev(x) if isinstance(x, np.ndarray) else x for x in args_b]
    try:
        call(*da)                                                # once before: the kernels are loaded
        empty_pool()
        guarded.bufs.clear()
        delay(sa)
        with torch.cuda.stream(sa):
            res_a = call(*da)
        witness, bw = plan_create(dkw, sb)                       # the pool's next block: A's, if A has given it back already
        with torch.cuda.stream(sb):
            res_b = call(*db)
        sb.synchronize()
        assert_busy(sa)                                          # A returned without a wait and was pending while B completed
        got_a = consume_on(sa, *res_a)
        plan_permute(witness, bw, dkw, dvw, ow, sb, True)        # A has run: over the witness's offsets, had they shared a block
        L.kh_shard_plan_destroy(witness)
        got_w = consume_on(sb, ow.k, ow.v)
        ow.check(*got_w, plan_expected(kw, vw, bw, True), "the witness plan")
        got_b = [t.cpu().numpy() for t in res_b]
        got_a = got_a if isinstance(got_a, list) else [got_a]
        for who, got, exp in (("A", got_a, exp_a), ("B", got_b, exp_b)):
            assert len(got) == len(exp)
            for i, (g, e) in enumerate(zip(got, exp)):
                e = np.asarray(e)
                assert g.view(e.dtype).tobytes() == e.tobytes(), "call %s, output %d" % (who, i)
        guarded.check()
    finally:
        torch.cuda.synchronize()


def edits_batch(seed, edits):
    B = Batch(7)                                                 # the same layout both times; the planted edits differ
    rng = random.Random(seed)
    for t in range(300):
        a = bases(B.rng, 10 + t % 40)
        b = sub(rng, a, rng.sample(range(len(a)), min(len(a), edits[t % len(edits)])))
        B.add([(a, b), (a, a)], rev=t & 1)
    return B


def test_chain_edits_scratch_outlives_the_queued_call(streams, guarded):
    a, b = edits_batch(1, [0, 1, 2, 5]), edits_batch(2, [1, 0, 3, 0])
    ra, rb = a.arrays(), b.arrays()
    assert [x.shape for x in ra] == [x.shape for x in rb] and a.n_chains == b.n_chains and not np.array_equal(ra[1], rb[1])
    exp_a, exp_b = EM.chain_edits_model(*ra, a.n_chains, 15), EM.chain_edits_model(*rb, b.n_chains, 15)
    assert not np.array_equal(exp_a[0], exp_b[0])
    queued_pair(streams, guarded, lambda *x: tuple(kh.chain_edits(*x, a.n_chains, 15)), ra, rb, exp_a, exp_b)


def test_select_chains_scratch_outlives_the_queued_call(streams, guarded):
    sizes = (0, 3, 64, 65, 200, 2100, 0)                         # both kernels; 2100 > 2048: sorted and swept over scratch
    a, b = SC.batch(sizes, "ties", "random", seed=21), SC.batch(sizes, "ties", "random", seed=22)
    assert [x.shape for x in a] == [x.shape for x in b]
    exp_a, exp_b = select_model(*a), select_model(*b)
    assert not np.array_equal(exp_a[0], exp_b[0])
    queued_pair(streams, guarded, lambda *x: tuple(kh.select_chains(*x)), a, b, exp_a, exp_b)


def test_pair_chains_returns_at_once_and_is_right_beside_a_second_call(streams, guarded):
    order = ("rs", "re", "rev", "score", "read_offsets", "tid", "use", "mapq")
    ta, tb = random_table(n_pairs=300, seed=9), random_table(n_pairs=300, seed=10)
    params = dict(min_ins=ta["min_ins"], max_ins=ta["max_ins"], unpaired_pen=ta["unpaired_pen"])
    a, b = [ta[k] for k in order], [tb[k] for k in order]
    queued_pair(streams, guarded, lambda *x: tuple(kh.pair_chains(*x, **params)), a, b, pair_model(*a, **params), pair_model(*b, **params))


def test_pack_rows_returns_at_once_and_is_right_beside_a_second_call(streams, guarded):
    def expected(case):
        text, lo, hi, dst, out_len = case
        return [np.frombuffer(bytes(FM.pack_rows(text.tobytes(), lo.tolist(), hi.tolist(), dst.tolist(), 10, bytearray(out_len))), dtype=np.uint8)]
    a, b = FC.pack_case(seed=3), FC.pack_case(seed=4)
    assert not np.array_equal(a[0], b[0])
    queued_pair(streams, guarded, lambda text, lo, hi, dst, out_len: (kh.pack_rows(text, lo, hi, dst, out_len, sep=10),), a, b, expected(a), expected(b))
