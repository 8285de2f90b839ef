"""GPU: the container contract of the Python wrappers -- what kind of array every public call returns for what kind of input.

Every wrapper that returns arrays is called with the same data as numpy arrays (the host form, the reference of the test) and as
    device          contiguous CUDA tensors
    host_strided    numpy views with a stride
    device_strided  CUDA tensor views with a stride
    cpu_tensor      CPU tensors: they go through numpy and numpy comes back
    side_stream     CUDA tensors, the call issued under torch.cuda.stream(s) and its results read on s
and every form must give the container kind, dtype (uint64 <-> int64, uint32 <-> int32, uint8, int32, bool), shape and device the
docstrings promise and the host form's values bit for bit.  Sizes are the smallest at which the edges live: 0, 1 and 65 keys or
anchors (one past a wavefront); texts of 0 bytes, k - 1 bases (no window) and 200 bases holding one N.  The values themselves are
pinned against the CPU models elsewhere in the suite; this file pins the plumbing around the C calls.  No wrapper refuses an empty
batch or an empty text in any form: each returns empty containers of the same kinds."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402
from kmerhash_amd import workloads as W  # noqa: E402
from stream_checks import to_dev  # noqa: E402

U64, U32, I32, U8, BOOL = (np.dtype(t) for t in (np.uint64, np.uint32, np.int32, np.uint8, np.bool_))
TORCH_OF = {U64: torch.int64, U32: torch.int32, I32: torch.int32, U8: torch.uint8, BOOL: torch.bool}
FORMS = ("device", "host_strided", "device_strided", "cpu_tensor", "side_stream")
SIZES = (0, 1, 65)
K, KWIDE, S_WIDE = 15, 35, 31


# ---- the forms of one argument ---------------------------------------------------------------------------------------------------
def strided(a):
    """the same values behind a stride: every second row of the rows repeated twice"""
    v = np.repeat(np.ascontiguousarray(a), 2, axis=0)[::2]
    assert len(v) < 2 or not v.flags.c_contiguous
    return v


def as_form(a, form):
    if form == "host" or not isinstance(a, np.ndarray):
        return a                                              # (not an array: a parameter, not a batch)
    if form == "host_strided":
        return strided(a)
    if form == "cpu_tensor":
        return to_dev(a).cpu()
    if form == "device_strided":
        t = to_dev(np.repeat(np.ascontiguousarray(a), 2, axis=0))[::2]
        assert len(t) < 2 or not t.is_contiguous()
        return t
    return to_dev(a)


def flat(r):
    """the arrays of a result in order (named tuples and nested tuples opened, None kept)"""
    if isinstance(r, tuple):
        return [x for part in r for x in flat(part)]
    return [r]


def outcome(call, args):
    """-> per output (container kind, dtype, shape, host copy made on the current stream)"""
    res = []
    for x in flat(call(*args)):
        if x is None:
            res.append(None)
        elif isinstance(x, torch.Tensor):
            res.append(("tensor:%s" % x.device, x.dtype, tuple(x.shape), x.cpu().numpy()))
        else:
            res.append((type(x).__name__, x.dtype, tuple(x.shape), x))
    return res


def same_bits(got, ref):
    return got.shape == ref.shape and np.array_equal(got if got.dtype == ref.dtype else got.view(ref.dtype), ref)


def check(name, call, args, dtypes, shapes=None):
    """call(*args) in every form.  dtypes: the numpy dtype of each output of the host form (None: the output is None); shapes: their
    expected shapes where the sizes alone give them (None entries: whatever the host form gave)"""
    bad = []
    shapes = shapes or [None] * len(dtypes)
    ref = None
    for form in ("host",) + FORMS:
        fargs = [as_form(a, form) for a in args]
        if form == "side_stream":
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                got = outcome(call, fargs)                    # (the host copies are made on s, inside)
            s.synchronize()
        else:
            got = outcome(call, fargs)
        on_host = form in ("host", "host_strided", "cpu_tensor")
        if len(got) != len(dtypes):
            bad.append("%s: %d outputs, expected %d" % (form, len(got), len(dtypes)))
            continue
        if ref is None:
            ref = [None if g is None else g[3] for g in got]
        for i, (g, dt, shp, r) in enumerate(zip(got, dtypes, shapes, ref)):
            if dt is None or g is None:
                if not (dt is None and g is None):
                    bad.append("%s[%d]: %r where %r was expected" % (form, i, g and g[:3], dt))
                continue
            kind, dtype, shape, val = g
            want = ("ndarray", dt) if on_host else ("tensor:cuda:0", TORCH_OF[dt])
            if (kind, dtype) != want:
                bad.append("%s[%d]: %s of %s, expected %s of %s" % (form, i, kind, dtype, *want))
            elif shp is not None and shape != tuple(shp):
                bad.append("%s[%d]: shape %s, expected %s" % (form, i, shape, tuple(shp)))
            elif not same_bits(val, r):
                bad.append("%s[%d]: values differ from the first form's (shape %s against %s)" % (form, i, shape, r.shape))
    assert not bad, "%s: %s" % (name, "; ".join(bad))


# ---- data ------------------------------------------------------------------------------------------------------------------------
def random_text(n, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].copy()


REF = random_text(400, 5)                                     # the text the indexes hold
QUERY = REF[60:260].copy()                                    # 200 bases of it, one of them no base
QUERY[97] = ord("N")
NKEYS = 80
KEYS = W.distinct_u64(NKEYS, seed=21)
VALS = np.arange(1, NKEYS + 1, dtype=np.uint32)
WKEYS = np.ascontiguousarray(np.stack([W.distinct_u64(NKEYS, seed=22), W.distinct_u64(NKEYS, seed=23)], axis=1))


def queries(n, wide=False):
    """n keys, hits and misses mixed"""
    hit, miss = (WKEYS, WKEYS + np.uint64(1)) if wide else (KEYS, W.distinct_u64(NKEYS, seed=31))
    both = np.concatenate([hit, miss])[np.random.default_rng(7).permutation(2 * NKEYS)]
    return np.ascontiguousarray(both[:n])


def text_of(size, k):
    return {"empty": QUERY[:0], "short": QUERY[:k - 1], "long": QUERY}[size].copy()


TEXT_SIZES = ("empty", "short", "long")


@pytest.fixture(scope="module")
def narrow():
    t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)
    assert t.insert(KEYS, VALS) == NKEYS
    yield t
    t.close()


@pytest.fixture(scope="module")
def wide():
    t = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8)
    assert t.insert(WKEYS, VALS) == NKEYS
    yield t
    t.close()


@pytest.fixture(scope="module")
def index():
    ix = kh.KmerPositionIndex(k=K, stranded=True)
    assert ix.build_sequences(REF) == len(REF) - K + 1
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def wide_index():
    ix = kh.WideKmerPositionIndex(k=KWIDE, s=S_WIDE, stranded=True)
    assert ix.build_sequences(REF) > 65
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def anchors(index):
    """(qpos, rpos, rev) of QUERY on the narrow index, host arrays: more than 65 of them"""
    q, r, v = index.anchors(QUERY)
    assert len(q) > 65 and q.dtype == U32 and v.dtype == U8
    return q, r, v


# ---- tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_table_lookups(narrow, wide, width, n):
    t, q = (narrow, queries(n)) if width == "narrow" else (wide, queries(n, wide=True))
    kshape = (None,) if width == "narrow" else (None, 2)
    check("%s.count" % width, t.count, [q], [U8], [(n,)])
    check("%s.find_values" % width, t.find_values, [q], [U32, U8], [(n,), (n,)])
    check("%s.find" % width, t.find, [q], [U64, U32])
    if n:
        fk, fv = t.find(q)
        assert fk.shape[1:] == kshape[1:] and len(fk) == len(fv) <= n and (n < 65 or 0 < len(fk) < n)


def test_count_and_find_values_write_into_the_callers_tensors(narrow):
    q = queries(65)
    dq = to_dev(q)
    out = torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    assert narrow.count(dq, out=out) is out and np.array_equal(out.cpu().numpy(), narrow.count(q))
    vals, found = torch.zeros(65, dtype=torch.int32, device="cuda"), torch.full((65,), 7, dtype=torch.uint8, device="cuda")
    rv, rf = narrow.find_values(dq, out_vals=vals, out_found=found, want_total=False)
    assert rv is vals and rf is found
    hv, hf = narrow.find_values(q)
    assert np.array_equal(vals.cpu().numpy().view(np.uint32), hv) and np.array_equal(found.cpu().numpy(), hf)


@pytest.mark.parametrize("picked", [0, 1, NKEYS])
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_select_values(narrow, wide, width, picked):
    t = narrow if width == "narrow" else wide
    lo, hi = {0: (5, 4), 1: (3, 3), NKEYS: (0, 0xFFFFFFFF)}[picked]
    kshape = (picked,) if width == "narrow" else (picked, 2)
    hk, hv = t.select_values(lo, hi)
    assert type(hk) is np.ndarray and type(hv) is np.ndarray and (hk.dtype, hv.dtype) == (U64, U32) and (hk.shape, hv.shape) == (kshape, (picked,))
    s = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), s):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            dk, dv = t.select_values(lo, hi, device=True)
            got = dk.cpu().numpy(), dv.cpu().numpy()
        assert (dk.dtype, dv.dtype) == (torch.int64, torch.int32) and (tuple(dk.shape), tuple(dv.shape)) == (kshape, (picked,))
        assert dk.device == dv.device == torch.device("cuda", 0)
        assert same_bits(got[0], hk) and same_bits(got[1], hv)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_to_vector(width, n):
    if width == "narrow":
        t, keys, kshape = kh.hashmap_robinhood_doubling(128, 0.35, 0.8), KEYS[:n], (n,)
    else:
        t, keys, kshape = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8), WKEYS[:n], (n, 2)
    try:
        if n:
            assert t.insert(to_dev(keys), to_dev(VALS[:n])) == n
        k, v = t.to_vector()
        assert type(k) is np.ndarray and type(v) is np.ndarray and (k.dtype, v.dtype) == (U64, U32) and (k.shape, v.shape) == (kshape, (n,))
        sk, sv = t.select_values(0, 0xFFFFFFFF)
        assert np.array_equal(k, sk) and np.array_equal(v, sv)
        assert sorted(map(tuple, k.reshape(n, len(kshape)).tolist())) == sorted(map(tuple, keys.reshape(n, len(kshape)).tolist()))
    finally:
        t.close()


@pytest.mark.parametrize("n", SIZES)
def test_hash_batch(n):
    check("hash_batch", kh.hash_batch, [queries(n)], [U64], [(n,)])
    check("hash_batch.lex_less", lambda q: kh.hash_batch(q, "farm", 1, 0, K), [queries(n)], [U64], [(n,)])
    check("hash_batch_wide", kh.hash_batch_wide, [queries(n, wide=True)], [U64], [(n,)])


# ---- text front ends -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", TEXT_SIZES)
def test_kmers_from_text(size):
    t, tw = text_of(size, K), text_of(size, KWIDE)
    check("kmers_from_sequence", lambda x: KM.kmers_from_sequence(x, K), [t], [U64])
    check("kmers_from_sequence.pos", lambda x: KM.kmers_from_sequence(x, K, with_positions=True), [t], [U64, U32])
    check("kmers128_from_sequence", lambda x: kh.kmers128_from_sequence(x, KWIDE), [tw], [U64])
    check("kmers128_from_sequence.pos", lambda x: kh.kmers128_from_sequence(x, KWIDE, with_positions=True), [tw], [U64, U32])
    if size != "empty":
        km, pos = KM.kmers_from_sequence(t.tobytes(), K, with_positions=True)          # bytes are host text
        assert same_bits(km, KM.kmers_from_sequence(t, K)) and km.ndim == 1 and len(pos) == len(km) == (0 if size == "short" else 200 - K + 1 - K)
        kw = kh.kmers128_from_sequence(tw, KWIDE)
        assert kw.shape == ((0 if size == "short" else 200 - KWIDE + 1 - KWIDE), 2)


def fastq_of(seq):
    """one record around the bases (none: no record)"""
    if len(seq) == 0:
        return seq
    return np.frombuffer(b"@r\n" + seq.tobytes() + b"\n+\n" + b"I" * len(seq) + b"\n", dtype=np.uint8).copy()


@pytest.mark.parametrize("size", TEXT_SIZES)
def test_kmers_from_fastq(size):
    t, tw = fastq_of(text_of(size, K)), fastq_of(text_of(size, KWIDE))
    check("kmers_from_fastq", lambda x: KM.kmers_from_fastq(x, K), [t], [U64])
    check("kmers_from_fastq.pos", lambda x: KM.kmers_from_fastq(x, K, with_positions=True), [t], [U64, U32])
    check("kmers128_from_fastq", lambda x: kh.kmers128_from_fastq(x, KWIDE), [tw], [U64])
    check("kmers128_from_fastq.pos", lambda x: kh.kmers128_from_fastq(x, KWIDE, with_positions=True), [tw], [U64, U32])


@pytest.mark.parametrize("size", TEXT_SIZES)
def test_samplers(size):
    t, tw = text_of(size, K), text_of(size, KWIDE)
    check("minimizers_from_sequence", lambda x: kh.minimizers_from_sequence(x, K, 5), [t], [U64, U32])
    check("minimizers_from_fastq", lambda x: kh.minimizers_from_fastq(x, K, 5), [fastq_of(t)], [U64, U32])
    check("syncmers_from_sequence", lambda x: kh.syncmers_from_sequence(x, K, 11), [t], [U64, U32])
    check("syncmers_from_fastq", lambda x: kh.syncmers_from_fastq(x, K, 11), [fastq_of(t)], [U64, U32])
    check("syncmers128_from_sequence", lambda x: kh.syncmers128_from_sequence(x, KWIDE, S_WIDE), [tw], [U64, U32])
    check("syncmers128_from_fastq", lambda x: kh.syncmers128_from_fastq(x, KWIDE, S_WIDE), [fastq_of(tw)], [U64, U32])
    if size != "empty":
        km, pos = kh.syncmers128_from_sequence(tw, KWIDE, S_WIDE)
        assert km.shape == (len(pos), 2) and (len(pos) > 0) == (size == "long")
        km, pos = kh.minimizers_from_sequence(t, K, 5)
        assert km.shape == pos.shape and (len(pos) > 0) == (size == "long")


@pytest.mark.parametrize("n", SIZES)
def test_syncmer_masks(n):
    km = KM.kmers_from_sequence(REF, K)[:n]
    kw = kh.kmers128_from_sequence(REF, KWIDE)[:n]
    assert len(km) == len(kw) == n
    check("is_syncmer", lambda x: kh.is_syncmer(x, K, 11), [km], [BOOL], [(n,)])
    check("is_syncmer128", lambda x: kh.is_syncmer128(x, KWIDE, S_WIDE), [kw], [BOOL], [(n,)])
    assert n < 65 or 0 < int(kh.is_syncmer(km, K, 11).sum()) < n


# ---- strand, anchors, chains, edits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_stamp_strand(n):
    pos = np.random.default_rng(3).integers(0, len(QUERY), n).astype(np.uint32)          # some windows hold the N or pass the end
    check("stamp_strand", lambda t, p: kh.stamp_strand(t, p, K), [QUERY, pos], [U32], [(n,)])
    stamped, invalid = kh.stamp_strand(to_dev(QUERY), to_dev(pos), K, count_invalid=True)
    assert stamped.dtype == torch.int32 and invalid == int((kh.stamp_strand(QUERY, pos, K) == KM.POS_INVALID).sum()) and (n < 65 or invalid > 0)


@pytest.mark.parametrize("n", SIZES)
def test_anchors_from_csr(index, n):
    if n:
        km, qpos = KM.kmers_from_sequence(QUERY, K, with_positions=True)
        km, sq = km[:n], kh.stamp_strand(QUERY, qpos[:n], K)
        offsets, positions = index.find(km)
    else:                                                         # the CSR of no query
        sq, offsets, positions = np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    assert len(positions) >= n
    check("anchors_from_csr", kh.anchors_from_csr, [sq, offsets, positions], [U32, U32, U8], [(len(positions),)] * 3)


@pytest.mark.parametrize("segments", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_chain_anchors_and_edits(anchors, n, segments):
    q, r, v = (a[:n].copy() for a in anchors)
    args = [q, r, v] + ([np.array([0, n // 2, n], dtype=np.uint64)] if segments else [])
    name = "chain_anchors.seg" if segments else "chain_anchors"
    check(name, lambda q, r, v, seg=None: kh.chain_anchors(q, r, v, K, seg, min_score=20), args, [I32, I32, I32, U32, U32, U32, I32],
          [(n,)] * 3 + [None] * 4)
    c = kh.chain_anchors(*args[:3], K, args[3] if segments else None, min_score=20)
    assert n < 65 or len(c.first) >= 1, "65 collinear anchors must give a chain"
    nc = len(c.first)
    check("chain_edits", lambda p, ch: kh.chain_edits(*(to_like(a, p) for a in (QUERY, REF, q, r, v)), p, ch, nc, K), [c.pred, c.chain],
          [I32, U32, U32], [(n,), (nc,), (nc,)])


def to_like(a, like):
    """host array `a` in the form of `like` (the fixed arguments of a call follow the form of the varied ones)"""
    if isinstance(like, torch.Tensor):
        return to_dev(a) if like.is_cuda else to_dev(a).cpu()
    return a


# ---- the index classes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_index_lookups(index, wide_index, width, n):
    if width == "narrow":
        ix, keys = index, np.concatenate([KM.kmers_from_sequence(REF, K)[:n // 2 + 1], queries(n)])[:n]
    else:
        ix, keys = wide_index, np.concatenate([kh.kmers128_from_sequence(REF, KWIDE)[:n // 2 + 1], queries(n, wide=True)])[:n]
    assert len(keys) == n
    check("%s_index.count" % width, ix.count, [keys], [U32], [(n,)])
    check("%s_index.find" % width, ix.find, [keys], [U64, U32], [(n + 1,), None])
    check("%s_index.find.offsets" % width, lambda x: ix.find(x, positions=False), [keys], [U64, None], [(n + 1,), None])
    check("%s_index.find.cap" % width, lambda x: ix.find(x, cap_out=4096), [keys], [U64, U32], [(n + 1,), None])
    check("%s_index.sampled" % width, ix.sampled, [keys], [BOOL], [(n,)])
    assert n < 65 or int(ix.count(keys).sum()) > 0


@pytest.mark.parametrize("size", TEXT_SIZES)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_index_text_queries(index, wide_index, width, size):
    ix, t = (index, text_of(size, K)) if width == "narrow" else (wide_index, text_of(size, KWIDE))
    check("%s_index.find_sequences" % width, ix.find_sequences, [t], [U32, U64, U32])
    check("%s_index.anchors" % width, ix.anchors, [t], [U32, U32, U8])
    chain_table = [U32, U8, U32, U32, U32, U32, U32, I32, U32, U32, U8, I32]          # ChainTable: 8 columns, the anchors, chain per anchor
    check("%s_index.chains" % width, lambda x: ix.chains(x, min_score=20), [t], chain_table)
    if size == "long":
        assert len(ix.anchors(t)[0]) > 0 and (width == "wide" or len(ix.chains(t, min_score=20).seg) > 0)
